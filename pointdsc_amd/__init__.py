"""pointdsc_amd -- MI355X-native (gfx950) implementation of PointDSC's test-time outlier-rejection
hot path behind the reference's ``PointDSC(...).forward(data) -> dict`` boundary.

Only what the path needs lives here:
  csrc/        hand-written HIP kernels + the C-ABI shared library ``libpointdsc_hip.so``
  _lib.py      ctypes binding of include/pointdsc_hip.h (fails loudly when the library is missing)
  model.py     ``PointDSC`` nn.Module: reference constructor, state_dict layout and forward contract
  ops.py       stage-level tensor wrappers (``rigid_transform_3d``, ``knn`` ...) over the C-ABI
  icp.py       the evaluation's optional ICP post-step (``icp_refine``, ``registration_icp``) on the device
  ransac.py    correspondence RANSAC (``ransac_correspondence``: the baseline's and the evaluation's ``--solver RANSAC``) on the device
  features.py  FPFH descriptors of a down-sampled cloud (neighbour lists, normals, SPFH, FPFH) on the device
  losses.py   the reference's training / validation losses (classification, spectral matching, transformation) on the device,
               with their gradients
  training.py  the differentiable spatial-consistency attention (``sc_attention``: device forward and backward behind a
               ``torch.autograd.Function``), the reference's ``NonLocalBlock`` built on it, the differentiable feature-similarity
               matrix (``feature_similarity``), the differentiable per-seed solver (``seed_solve``), the fused train-mode point-wise
               layer (``conv_bn_relu``), the train path's plain linears (``linear_rows``, ``qkv_projection``,
               ``classification_head``), the train()-mode forward (``train_forward``) and ``TrainablePointDSC``
  optim.py     the trainer's update on the device: ``DeviceAdam`` / ``DeviceSGD`` (finite-gradient guard, update and skip decision
               in a handful of multi-tensor launches, nothing read back)
  multiway.py  the multiway driver's edge step (information matrix + overlap gate, voxel down-sampling, multi-scale ICP) and its
               pose-graph optimisation (node chain, LM with line process, edge pruning) on the device
  sharding.py  one-process-per-GPU sharding of pair batches + the single RCCL pose gather
  synthetic.py seeded synthetic correspondence sets / weights (tests + bench)
"""
from .correspondences import CorrPool, build_correspondences_batch  # noqa: F401
from .features import (compute_fpfh_feature, estimate_normals, extract_fpfh_features, fpfh_descriptors,  # noqa: F401
                       hybrid_neighbours, voxel_down_sample_with_normals)
from .icp import icp_refine, registration_icp  # noqa: F401
from .ransac import ransac_correspondence  # noqa: F401
from .losses import ClassificationLoss, SpectralMatchingLoss, TransformationLoss  # noqa: F401
from .model import PointDSC  # noqa: F401
from .training import (NonLocalBlock, TrainablePointDSC, classification_head, conv_bn_relu, feature_similarity,  # noqa: F401
                       linear_rows, qkv_projection, sc_attention, seed_solve, train_forward)
from .optim import DeviceAdam, DeviceSGD  # noqa: F401
from .multiway import (align, global_optimization, information_matrix, local_refinement, loop_closure_edge,  # noqa: F401
                       multi_scale_icp, pose_graph_nodes, voxel_down_sample)

__all__ = ["PointDSC", "icp_refine", "registration_icp", "information_matrix", "voxel_down_sample", "loop_closure_edge",
           "multi_scale_icp", "local_refinement", "align", "hybrid_neighbours", "estimate_normals", "compute_fpfh_feature",
           "fpfh_descriptors", "voxel_down_sample_with_normals", "extract_fpfh_features", "pose_graph_nodes", "global_optimization",
           "ClassificationLoss", "SpectralMatchingLoss", "TransformationLoss", "NonLocalBlock", "sc_attention",
           "TrainablePointDSC", "train_forward", "feature_similarity", "seed_solve", "conv_bn_relu",
           "linear_rows", "qkv_projection", "classification_head", "build_correspondences_batch", "CorrPool", "ransac_correspondence",
           "DeviceAdam", "DeviceSGD"]

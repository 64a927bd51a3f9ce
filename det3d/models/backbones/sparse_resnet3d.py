"""configs/models/backbone/3d_sparse_resnet18.yaml -> `_target_: det3d.models.backbones.sparse_resnet3d.SparseResNet3D` (sparse 3-D HIP kernels)."""
from pillarnext_amd.sparse3d import SparseBasicBlock3d, SparseConv3d, SparseConv3dBlock, SparseResNet3D  # noqa: F401

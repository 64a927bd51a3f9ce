"""configs/dataset/base/base_det_train.yaml -> `_target_: det3d.datasets.pipelines.assign.AssignLabel`."""
from pillarnext_amd.assign import AssignLabel  # noqa: F401

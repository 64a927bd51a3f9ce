"""configs/dataset/preprocess/augmentation.yaml -> `_target_: det3d.datasets.pipelines.augmentation.{Rotation, Scaling, Translation, Flip}`."""
from pillarnext_amd.augment import Flip, Rotation, Scaling, Translation  # noqa: F401

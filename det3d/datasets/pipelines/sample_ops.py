"""The experiment YAMLs -> `_target_: det3d.datasets.pipelines.sample_ops.{DataBaseSamplerV2, DBFilterByMinNumPoint}`."""
from pillarnext_amd.augment import BatchSampler, DataBaseSamplerV2, DBFilterByMinNumPoint  # noqa: F401

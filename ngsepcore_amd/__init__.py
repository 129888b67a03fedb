"""ngsepcore_amd -- MI355X-native drop-in for NGSEP's SNV pileup-calling path.

The compute path is libngsep_amd.so (HIP kernels for gfx950 behind the C ABI in
include/ngsep_gpu.h); this package is the host-side mirror of the reference interface.
"""
from ._lib import LIB_PATH, NgsepError, load  # noqa: F401
from .discovery import (BasePairQualityStatisticsCalculator, CalledSite, CoverageStatisticsCalculator, GpuPileupSession,  # noqa: F401
                        MultisampleVariantsDetector, PopulationSite, RelativeAlleleCountsCalculator,
                        SingleSampleVariantsDetector, default_params)

__all__ = ["GpuPileupSession", "BasePairQualityStatisticsCalculator", "CoverageStatisticsCalculator", "RelativeAlleleCountsCalculator", "SingleSampleVariantsDetector", "MultisampleVariantsDetector", "PopulationSite", "CalledSite", "NgsepError", "default_params",
           "load", "LIB_PATH"]

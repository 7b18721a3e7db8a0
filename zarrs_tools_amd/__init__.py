"""zarrs_tools_amd — MI355X-native zarrs_filter per-chunk transform path.

The compute lives in libzarrs_tools_amd.so (hand-written HIP kernels for gfx950 behind the C ABI
in include/zarrs_tools_amd.h). This package is the thin host-side mirror of the reference's
filter-operator surface (LDeakin/zarrs_tools src/filter/) used by tests and bench.py.
Importing it loads the library; if it is missing the import fails loudly (no CPU fallback).
"""
from ._abi import DTYPES, FilterError, InvalidParameters, UnsupportedDataType, lib

lib()  # fail at import time if the native library is absent

from .filter import (  # noqa: E402
    ARITHMETIC_OPERATORS,
    Arithmetic,
    ArraySubset,
    ArraySubsetOverlap,
    Clamp,
    chunk_occupancy,
    Compare,
    ConnectedComponents,
    Context,
    Crop,
    DeviceArray,
    DistanceTransform,
    Downsample,
    Equal,
    Gaussian,
    GradientMagnitude,
    GuidedFilter,
    Histogram,
    LabelSizeFilter,
    LabelStatistics,
    Maximum,
    Median,
    Minimum,
    PointwiseProgram,
    Range,
    RankFilter,
    Reconstruction,
    Reencode,
    ReplaceValue,
    Rescale,
    SummedAreaTable,
    Watershed,
    combine_compares,
    combine_histograms,
    combine_label_statistics,
    combine_ranges,
    default_context,
    dtype_of,
    label_size_filter,
    label_statistics,
    pyramid,
    pyramid_level_shapes,
    synth_step_noise_f32,
    synth_u16,
    synth_box,
    torch_dtype,
)
from .shard import OctantAssignment, SlabAssignment, octant_assignment, slab_assignment  # noqa: E402

__all__ = [
    "ArraySubset", "ArraySubsetOverlap", "Context", "DeviceArray", "Downsample", "DTYPES",
    "FilterError", "Gaussian", "GradientMagnitude", "GuidedFilter", "InvalidParameters", "SlabAssignment", "SummedAreaTable",
    "UnsupportedDataType",
    "Clamp", "Crop", "Equal", "PointwiseProgram", "Reencode", "ReplaceValue", "Rescale",
    "default_context", "dtype_of", "lib", "octant_assignment", "OctantAssignment", "pyramid",
    "pyramid_level_shapes", "slab_assignment",
    "synth_step_noise_f32", "synth_u16", "synth_box", "torch_dtype",
    "Histogram", "Range", "combine_histograms", "combine_ranges",
    "Compare", "combine_compares",
    "chunk_occupancy",
    "RankFilter", "Median", "Minimum", "Maximum",
    "Arithmetic", "ARITHMETIC_OPERATORS",
    "ConnectedComponents",
    "DistanceTransform",
    "LabelStatistics", "LabelSizeFilter", "combine_label_statistics", "label_statistics",
    "label_size_filter",
    "Reconstruction",
    "Watershed",
]

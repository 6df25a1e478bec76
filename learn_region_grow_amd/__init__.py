"""learn_region_grow_amd -- MI355X-native LRGNet region-grow inference path.

Host side (Python) mirrors the reference's operator interface for this path
(``LrgNet`` -> ``LrgNetHIP``, the ``test_region_grow.py`` loop -> ``RegionGrower``,
``tf_ops/grouping`` -> ``grouping``, ``tf_ops/sampling`` -> ``sampling``,
``tf_ops/3d_interpolation`` -> ``interpolate``, ``benchmarks.py`` -> ``baselines``,
``MCPNet`` / ``test_mcpnet.py`` -> ``mcpnet``) and drives hand-written HIP kernels for gfx950
through the C-ABI library ``liblrg_hip.so`` (include/lrg_hip.h).
"""
__version__ = "0.1.0"

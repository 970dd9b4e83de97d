"""harmonypy_amd -- MI355X-native Harmony iteration engine.

Drop-in for the hot path of slowkow/harmonypy: ``run_harmony`` / ``Harmony`` keep the
reference's signatures (harmonypy/__init__.py:1-4, harmony.py:49-67, 218-229); the
``harmonize()`` loop runs as hand-written HIP kernels for gfx950 behind a C ABI
(include/hmx.h, harmonypy_amd/libhmx.so).  ``compute_lisi`` (lisi.py:24-66) is the
reference's integration metric on the same device.  ``map_query`` places new cells onto a finished reference
(``HarmonyReference``) without a new run; ``knn_predict`` transfers the reference's labels to them by a vote of their
nearest reference cells (``knn_query``: the neighbours alone).  ``ClusterMoments`` and ``HarmonyQuery.mapping_score`` /
``cluster_mapping_score`` say how well the query landed: Mahalanobis distances from the reference's clusters.
"""
from .harmony import Harmony, run_harmony, BatchCodes  # noqa: F401
from .dist import Shard  # noqa: F401
from .lisi import compute_lisi  # noqa: F401
from .mapping import HarmonyReference, map_query  # noqa: F401
from .knn import knn_predict, knn_query  # noqa: F401
from .confidence import ClusterMoments  # noqa: F401

__version__ = "0.4.0"


def engine_version() -> str:
    """Identity of the kernel set in the loaded libhmx.so: the build id ``_build.py`` computed from csrc/ and hmx.h
    (``hmx_build_id()``).  profiles/*_pmc_hbm.json name the build their counters were collected on and bench.py only
    quotes counter-derived traffic for the build that is running -- nothing here is maintained by hand."""
    from . import _capi
    return _capi.build_id()


__all__ = ["Harmony", "run_harmony", "BatchCodes", "Shard", "compute_lisi", "map_query", "HarmonyReference", "knn_predict", "knn_query", "ClusterMoments", "__version__", "engine_version"]

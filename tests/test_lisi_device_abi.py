"""compute_lisi on device tensors and up to 320 features, what can be checked without a GPU: the new C entry point is
declared and exported, and the built library holds the neighbour-search instances above 208 features (KS16 14..20, every
candidate-list size) and the typed loaders, none of which spills, uses scratch or declares more LDS than a CU has."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_audit  # noqa: E402

from harmonypy_amd import _capi  # noqa: E402

LIB = _capi.LIB_PATH
needs_lib = pytest.mark.skipif(not (kernel_audit.tools_available() and os.path.exists(LIB)),
                               reason="needs the ROCm LLVM tools and a built libhmx.so")

CAPS = (256, 1024, 4096)            # candidate-list sizes (hmx_lisi.hip, lisi_list_cap)
WAVES = 4                           # LISI_KNN_WAVES
CU_LDS = 160 * 1024


def test_device_entry_point_is_declared_next_to_the_device_io():
    hdr = open(os.path.join(ROOT, "include", "hmx_device_io.h")).read()
    assert re.search(r"\bint hmx_compute_lisi_device\s*\(", hdr)
    assert "hmx_compute_lisi_device" in _capi.DEVICE_IO_EXPORTS
    assert "hmx_compute_lisi_device" not in _capi.EXPORTS
    # hmx.h keeps its declared set (the ABI stays at 8: an added symbol only)
    assert "hmx_compute_lisi_device" not in set(re.findall(r"\b(hmx_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "hmx.h")).read()))
    assert _capi.HMX_ABI_VERSION == 8


@pytest.mark.skipif(not os.path.exists(LIB), reason="needs a built libhmx.so")
def test_device_entry_point_is_exported():
    lib = _capi.load()
    assert hasattr(lib, "hmx_compute_lisi_device")
    assert len(lib.hmx_compute_lisi_device.argtypes) == 14
    assert lib.hmx_abi_version() == 8


@pytest.fixture(scope="module")
def lisi_rows():
    return {r["name"]: r for r in kernel_audit.audit(LIB, "lisi")}


@needs_lib
@pytest.mark.parametrize("ks16", range(14, 21))
def test_wide_search_instances_exist_without_spills(lisi_rows, ks16):
    for cap in CAPS:
        name = f"_ZN12_GLOBAL__N_110k_lisi_knnILi{ks16}ELi1ELi{cap}EEEv11LisiKnnArgs"
        assert name in lisi_rows, f"k_lisi_knn<{ks16}, 1, {cap}> missing"
        r = lisi_rows[name]
        assert r["vgpr_spill_count"] == 0, f"{name}: {r['vgpr_spill_count']} spilled VGPRs"
        assert r["private_segment_fixed_size"] == 0 and r.get("scratch", 0) == 0, f"{name} uses scratch"
        # static staging buffers + the dynamic sort scratch (waves x cap x 8 bytes) fit the CU's LDS
        assert r["group_segment_fixed_size"] + WAVES * cap * 8 <= CU_LDS, name
        # 256-entry lists: two workgroups of four waves per CU, so at most 256 registers per lane
        if cap == 256:
            assert r["vgpr_count"] <= 256, name
        assert r["mfma"] >= 4 * ks16                    # the tile products stay on the matrix cores


@needs_lib
def test_loaders_for_every_dtype_do_not_spill(lisi_rows):
    loads = [r for n, r in lisi_rows.items() if "k_lisi_load" in n]
    assert len(loads) == 4                                     # float32, float16, bfloat16, float64
    for r in loads:
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r["name"]


@needs_lib
def test_wide_search_has_no_register_touched_in_flight():
    hz = kernel_audit.inflight_hazards(LIB, "k_lisi")
    wide = {k: v for k, v in hz.items() if re.search(r"k_lisi_knnILi(1[4-9]|20)E", k)}
    assert len(wide) == 7 * len(CAPS)
    assert not {k: v for k, v in hz.items() if v}

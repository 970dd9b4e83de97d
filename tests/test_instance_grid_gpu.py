"""Every compiled instance of the iteration kernels against float64 (tests/instance_grid.py, tests/step_reference.py).

One case per grid row: an engine on the device update order runs init_cluster, then twice one round + the ridge; the
library's launch census (include/hmx_census.h) must hold every instance the row is in the grid for, the counters must
name the pipe, the tile map and the persistent sweep the row expects, and every step is held against its float64
evaluation FROM THE ENGINE'S OWN INPUT to that step (Y from the R before the round, the new R from the engine's Y, Z_corr
from the engine's R), so one kernel family's error never enters another's check.

Bars (profiles/instance_grid_errors.txt has the per-row figures).  Every compared quantity also gets its ANCHOR error: the
same step from the same inputs in the arithmetic the kernel is designed to have (step_reference.anchor_*: the six-product
bf16 emulation or fp32 accumulation of the f32-input matrix instruction; fp32 NumPy with the float64 solve for the ridge),
computed here on the CPU and written to the report with the engine's.
  * Z_corr, Z_cos: relative Frobenius and max-abs / max |ref| error <= instance_grid.BAR_FACTORS x the anchor's
    (1.25 x r_max, the largest engine / anchor ratio of two runs of the grid: 3.2 narrow, 2.6 wide, 9.6 generic for Z_corr).
  * R, Y: a factor would have to lie between 1.25 x r_max and 0.8 x s_min, the smallest (one product dropped) / anchor
    ratio of tests/test_instance_grid_cpu.py; none does.  R: r_max 4.98 (bf16-pipe rows alone 3.3 / 4.0) against s_min 3.33
    (l.h), 5.65 (m.m), 1.70 (h.l) -- the matrix instruction's own accumulation and the exp2 / log2 approximations are
    not in the anchor.  Y: r_max 1.44, s_min 0.72: the fp32 rounding of Y hides a dropped product of the R^T.Z pass.  They keep
    the absolute bars of the direct A/B tests (instance_grid.R_BARS, Y_BAR), here against float64 (measured: max |dR| <=
    3.5e-6 narrow, 6.6e-6 wide and generic, relative Frobenius <= 3.1e-6; max |dY| <= 1.8e-7); Y also its factor on the relative Frobenius error.
  * O, the cluster masses and the objective terms are fp64 sums inside the engine: O and the masses keep the bars of the
    step-level oracle test (rtol 1e-4, atol 3e-4: test_cluster_round_matches_oracle), the three objective terms the 2e-6
    relative of the A/B tests (measured <= 4.3e-7).
"""
import json
import os

import numpy as np
import pytest

import instance_grid as ig
import step_reference as sr

pytestmark = pytest.mark.gpu

F = ig.BAR_FACTORS
SEED = 11


def _report(line):
    path = os.environ.get("HMX_GRID_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


@pytest.mark.parametrize("row", ig.ROWS, ids=[r["id"] for r in ig.ROWS])
def test_grid_row_against_float64(row, monkeypatch):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import quick_centroids, synthetic_dataset
    from harmonypy_amd import _capi, harmony as H
    N, d, K, B, facts = row["N"], row["d"], row["K"], row["B"], row["facts"]
    for name in ig.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HMX_UPDATE_ORDER", "device")
    for name, value in row["env"].items():
        monkeypatch.setenv(name, value)
    Z, meta = synthetic_dataset(N, d, B, K, seed=3)
    Y0 = quick_centroids(Z, K, seed=3, sample=4000)
    batch = meta["batch"].str[1:].astype(int).to_numpy()
    _capi.launch_census(True)
    try:
        ho = H.run_harmony(Z, meta, ["batch"], verbose=False, _y0=Y0, nclust=K, max_iter_harmony=0, random_state=SEED,
                           block_size=row["block_size"])
        assert ho.update_order == "device" and ho._n_blocks == row["nblk"]
        Pr_b, theta, sigma, lamb = ho.Pr_b, ho.theta, ho.sigma, ho.lamb
        perm = sr.device_perm_source(N, SEED)
        rtz_products = "six" if facts["rtz_bf16"] else None
        gemm_products = "six" if facts["bf16"] else None
        figures = dict(id=row["id"])
        failures = []

        def check(what, got, ref, anchor):
            e, a = sr.errors(got, ref), sr.errors(anchor, ref)
            q = what.split(".")[0]
            figures[what] = dict(engine=e, anchor=a, max_abs=float(np.abs(got - ref).max()))
            regime = facts["regime"]
            if q == "R":                                              # [(measure, bar, how)], measure 0: relF, 1: max
                bars = [(0, ig.R_BARS[regime][0], "absolute"), (1, ig.R_BARS[regime][1] / float(np.abs(ref).max()), "absolute")]
            else:
                bars = [(i, f * a[i], f"{f} x anchor") for i, f in enumerate(F[q][regime]) if f is not None]
                if q == "Y":
                    bars.append((1, ig.Y_BAR / float(np.abs(ref).max()), "absolute"))
            print(f"{row['id']} {what}: relF {e[0]:.2e} ({e[0] / a[0]:.2f} anchors) max {e[1]:.2e} ({e[1] / a[1]:.2f} anchors)")
            for kind, bar, how in bars:
                if not e[kind] <= bar:
                    failures.append(f"{what} {('relF', 'max')[kind]}: engine {e[kind]:.3e} > bar {bar:.3e} ({how}; anchor {a[kind]:.3e})")

        for it in range(2):
            R0, Zc = ho.R, ho.Z_cos
            assert R0.shape == (N, K) and np.isfinite(R0).all()
            ho.cluster(_rounds=1)
            Y, R1 = ho.Y, ho.R
            assert Y.shape == (d, K) and R1.shape == (N, K) and ho.R.shape[1] == K
            assert np.isfinite(Y).all() and np.isfinite(R1).all()
            check(f"Y.{it}", Y, sr.centroids(Zc, R0), sr.anchor_centroids(Zc, R0, rtz_products))
            blocks = sr.blocks_of(perm(N), row["block_size"])
            ref = sr.sweep(Zc, Y, R0, batch, Pr_b, theta, sigma, blocks)
            anchor = sr.sweep(Zc, Y, R0, batch, Pr_b, theta, sigma, blocks, scale=sr.anchor_scale(Zc, Y, sigma, gemm_products))
            check(f"R.{it}", R1, ref["R"], anchor["R"])
            np.testing.assert_allclose(R1.sum(axis=1), 1.0, atol=3e-6)
            mass = ho._engine.get(_capi.HMX_T_MASS).reshape(-1)
            terms = {n: getattr(ho, f"objective_kmeans_{n}")[-1] * N / 2000.0 for n in ("dist", "entropy", "cross")}
            figures[f"sums.{it}"] = dict(O=float(np.abs(ho.O - ref["O"]).max()), mass=float(np.abs(mass - ref["mass"]).max()),
                                         **{n: abs(terms[n] - ref[n]) / abs(ref[n]) for n in terms})
            np.testing.assert_allclose(ho.O, ref["O"], rtol=1e-4, atol=3e-4, err_msg=f"O round {it}")
            np.testing.assert_allclose(mass, ref["mass"], rtol=1e-4, atol=3e-4, err_msg=f"cluster masses round {it}")
            for name in terms:                                            # (the A/B tests' 2e-6; measured <= 4.3e-7 over the grid)
                np.testing.assert_allclose(terms[name], ref[name], rtol=2e-6, err_msg=f"objective term {name} round {it}")
            Zo = ho.Z_orig
            ho.moe_correct_ridge()
            Zcorr, Zcos = ho.Z_corr, ho.Z_cos
            assert Zcorr.shape == (N, d) and np.isfinite(Zcorr).all() and np.isfinite(Zcos).all()
            r_corr, r_cos = sr.ridge(Zo, R1, batch, lamb)
            a_corr, a_cos = sr.anchor_ridge(Zo, R1, batch, lamb)
            check(f"Z_corr.{it}", Zcorr, r_corr, a_corr)
            check(f"Z_cos.{it}", Zcos, r_cos, a_cos)
        census = {ig.instance_name(s) for s in _capi.launch_census()}
        cnt = ho._engine.counters()
        figures["counters"] = {k: v for k, v in cnt.items() if k != "peer_box"}
        figures["census"] = sorted(c for c in census if c and ig.family(c) in ig.FAMILIES)
        _report(figures)
    finally:
        _capi.launch_census(False)
    missing = row["expect"] - census
    assert not missing, f"not launched: {sorted(missing)}; launched {figures['census']}"
    assert cnt["sweep_fallbacks"] == 0, cnt
    assert cnt["sweeps_bf16_pipe"] == (2 if facts["bf16"] else 0), cnt
    assert (cnt["rtz_bf16_pipe"] >= 2) if facts["rtz_bf16"] else (cnt["rtz_bf16_pipe"] <= 2), cnt     # (the ridge pass of a wide row may take k_rtzw2b where the round's cannot)
    assert cnt["sweeps_group_affine"] == (2 if facts["ga"] else 0), cnt
    if facts["ga"]:
        assert cnt["sweep_group_affine_wgs"] >= 3, cnt                    # a count field of the hand-off has two contributors
    assert cnt["sweeps_wide_persistent"] == (2 if facts["persistent"] and facts["regime"] == "wide" else 0), cnt
    assert cnt["rtz_presplit_z"] == (2 if facts["presplit"] else 0), cnt
    assert not failures, "; ".join(failures)

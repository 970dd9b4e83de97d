"""The instance grid without a GPU: the rows cover every compiled instance, step_reference is the oracle's algorithm,
and the float64 bars separate a kernel with a dropped product from a right one."""
import os
import sys
import tempfile

import numpy as np
import pytest

import instance_grid as ig
import step_reference as sr
from conftest import assert_z_close, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_audit  # noqa: E402

LIB = os.path.join(ROOT, "harmonypy_amd", "libhmx.so")


def test_instance_names_from_mangled_symbols():
    assert ig.instance_name("_Z7k_roundILi5ELi16ELb1EEv9RoundArgs") == "k_round<5,16,true>"
    assert ig.instance_name("_Z8k_rtzw2bILi11ELi5ELb0EEv8Rtz3Args") == "k_rtzw2b<11,5,false>"
    assert ig.instance_name("_Z13k_rtz3_finish14Rtz3FinishArgs") == "k_rtz3_finish"
    assert ig.instance_name("_ZN12_GLOBAL__N_18k_mscoreE10MScoreArgs") is None


@pytest.mark.skipif(not (kernel_audit.tools_available() and os.path.exists(LIB)), reason="needs the ROCm LLVM tools and a built libhmx.so")
def test_rows_and_unreachable_are_exactly_the_compiled_instances():
    """Every instance of the iteration's kernel families in the built library is in some row's `expect` (k_kmeans_step:
    in the device Lloyd test's parameters) or in UNREACHABLE with the dispatch predicate that excludes it, and nothing is
    in both: a new instance without a grid row fails here."""
    names = set()
    with tempfile.TemporaryDirectory() as wd:
        for co in kernel_audit.extract_code_objects(LIB, wd):
            names |= set(kernel_audit.kernel_metadata(co))
    compiled = {i for i in map(ig.instance_name, names) if i and ig.family(i) in ig.FAMILIES}
    covered = ig.covered()
    assert len(compiled) >= 365
    assert not (covered & set(ig.UNREACHABLE)), sorted(covered & set(ig.UNREACHABLE))
    assert covered | set(ig.UNREACHABLE) == compiled, (sorted(compiled - covered - set(ig.UNREACHABLE)), sorted((covered | set(ig.UNREACHABLE)) - compiled))
    assert len(ig.UNREACHABLE) <= 30 and all(len(why) > 40 for why in ig.UNREACHABLE.values())


def test_unreachable_instances_are_excluded_by_the_dispatch_over_all_shapes():
    """No shape (d, K up to the library's 320, 1..64 update blocks) under any row's switches selects an UNREACHABLE
    instance in dispatch() -- the restated predicates and the list agree."""
    envs = [dict(t) for t in {tuple(sorted(r["env"].items())) for r in ig.ROWS}]
    hit = set()
    for env in envs:
        for d in list(range(1, 70)) + list(range(70, 321, 5)) + [80, 96, 112, 208, 209]:
            for K in list(range(1, 321, 4)) + [16 * m for m in range(1, 21)]:
                for nblk in (1, 10, 16, 17, 20, 33, 40, 44, 45, 60, 64):
                    hit |= ig.dispatch(d, K, nblk, env)[0] & set(ig.UNREACHABLE)
    assert not hit, sorted(hit)


def test_rows_have_the_sizes_the_hand_off_needs():
    for r in ig.ROWS:
        assert ig.n_blocks(r["block_size"]) == r["nblk"], r["id"]
        per_block = int(r["N"] * r["block_size"])
        assert per_block * (r["nblk"] - 1) < r["N"], r["id"]
        if r["facts"]["regime"] == "narrow":
            assert per_block >= 400 and r["B"] == 2                   # ~ 25 tiles per block, two workgroups for the larger batch
        elif r["facts"]["regime"] == "wide":
            assert per_block // 16 >= 33 and r["B"] == 3              # more than one 16-tile chunk per block and group run


@pytest.mark.parametrize("case", ["pbmc_default", "synth_small_steps"])
def test_step_reference_is_the_oracles_algorithm(case):
    """One round + one ridge from the same state: step_reference (float64) against OracleHarmony (the reference's fp32),
    within the tolerances tests/test_oracle_golden.py gives the oracle against the goldens (R / O / E / Y: rtol 5e-4,
    atol 2e-5; Z: 1e-4 relative Frobenius and max-abs; objectives rtol 2e-5)."""
    from oracle.harmony_oracle import OracleHarmony, prepare_inputs
    data, meta, vars_use, kw, g = load_case(case)
    p = prepare_inputs(data, meta, vars_use, **{k: kw[k] for k in ("theta", "lamb", "sigma", "nclust", "tau") if k in kw})
    N = meta.shape[0]
    order = np.random.default_rng(5).permutation(N)
    oo = OracleHarmony(p["Z"], p["phi"], p["Pr_b"], p["sigma"], p["theta"], p["lamb"], K=p["K"], run=False,
                       block_size=kw.get("block_size", 0.05), perm_source=lambda n: order, forced_rounds=[1])
    oo.init_cluster(0, g["Y0"])
    R0, Zc = oo.R.T.copy(), oo.Z_cos.T.copy()
    batch = np.argmax(p["phi"], axis=0)
    oo.cluster()
    Y = sr.centroids(Zc, R0)
    np.testing.assert_allclose(Y, oo.Y, rtol=5e-4, atol=2e-5)
    ref = sr.sweep(Zc, oo.Y, R0, batch, p["Pr_b"], p["theta"], p["sigma"], sr.blocks_of(order, kw.get("block_size", 0.05)))
    np.testing.assert_allclose(ref["R"], oo.R.T, rtol=5e-4, atol=2e-5)
    np.testing.assert_allclose(ref["O"], oo.O, rtol=5e-4, atol=2e-4)
    np.testing.assert_allclose(np.outer(ref["mass"], p["Pr_b"]), oo.E, rtol=5e-4, atol=2e-4)
    for name in ("dist", "entropy", "cross"):
        np.testing.assert_allclose(ref[name] * 2000.0 / N, getattr(oo, f"objective_kmeans_{name}")[-1], rtol=2e-5)
    R1, Zo = oo.R.T.copy(), oo.Z_orig.T.copy()
    oo.moe_correct_ridge()
    Z_corr, Z_cos = sr.ridge(Zo, R1, batch, p["lamb"])
    assert_z_close(Z_corr, oo.Z_corr.T, what="Z_corr")
    assert_z_close(Z_cos, oo.Z_cos.T, what="Z_cos")
    a_corr, a_cos = sr.anchor_ridge(Zo, R1, batch, p["lamb"])
    assert_z_close(a_corr, Z_corr, tol=1e-5, what="fp32 anchor of Z_corr")


def _bf16_shapes():
    """(d, K, B) of every row whose sweep or round pass runs on the bf16 pipe, once each"""
    seen = {}
    for r in ig.ROWS:
        if r["facts"]["bf16"] or r["facts"]["rtz_bf16"]:
            seen.setdefault((r["d"], r["K"], r["B"]), r)
    return list(seen.values())


@pytest.mark.parametrize("row", _bf16_shapes(), ids=lambda r: f"d{r['d']}-K{r['K']}")
def test_a_dropped_product_against_the_bars(row):
    """For every (d, K) the grid runs on the bf16 pipe: the CPU emulation of the distance GEMM and of R^T.Z with ONE product
    of the six dropped (l.h, h.l, m.m), against float64 and against the six-product anchor, on 2 000 cells of the row's
    population.  Printed for every shape: the (mutation error) / (anchor error) ratios that profiles/instance_grid_errors.txt
    quotes as s_min.  Asserted: on the narrow shapes a dropped l.h or m.m product moves some R entry by more than the narrow
    rows' bar on max |dR| (instance_grid.R_BARS) -- the GPU test fails such a kernel.  NOT separated by the bars, and not
    asserted: h.l (1.7 .. 3 anchors), the wide rows' 3e-5 (a dropped l.h is 1 .. 2e-5 there), and Y, whose fp32 rounding
    hides a dropped product of the R^T.Z pass (ratios 0.7 .. 5)."""
    from bench import synthetic_dataset
    from test_split_gemm import SIX
    d, K, B = row["d"], row["K"], row["B"]
    n = 2000
    Z, meta = synthetic_dataset(n, d, B, K, seed=3)
    batch = meta["batch"].str[1:].astype(int).to_numpy()
    Zc = (Z / np.linalg.norm(Z.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(K * 1000 + d)
    Y = Zc[rng.choice(n, K, replace=False)].T + 0.1 * rng.standard_normal((d, K)).astype(np.float32)   # centroids near cells
    Y = (Y / np.linalg.norm(Y.astype(np.float64), axis=0)).astype(np.float32)
    sigma = np.full(K, 0.1, np.float32)
    Pr_b = (np.bincount(batch, minlength=B) / n).astype(np.float32)
    theta = np.full(B, 2.0, np.float32)
    R0 = sr.anchor_scale(Zc, Y, sigma, None)
    blocks = sr.blocks_of(np.random.default_rng(1).permutation(n), 0.05)
    sweep = lambda scale=None: sr.sweep(Zc, Y, R0, batch, Pr_b, theta, sigma, blocks, scale=scale)["R"]
    R_ref, Y_ref = sweep(), sr.centroids(Zc, R0)
    R_six = sweep(sr.anchor_scale(Zc, Y, sigma, "six"))
    aR, aY = sr.errors(R_six, R_ref), sr.errors(sr.anchor_centroids(Zc, R0, "six"), Y_ref)
    assert np.abs(R_six - R_ref).max() <= ig.R_BARS[row["facts"]["regime"]][1] / 2          # the right kernel is well inside the bar
    for drop in [("l", "h"), ("h", "l"), ("m", "m")]:
        products = [p for p in SIX if p != drop]
        R_mut = sweep(sr.anchor_scale(Zc, Y, sigma, products))
        mR, mY = sr.errors(R_mut, R_ref), sr.errors(sr.anchor_centroids(Zc, R0, products), Y_ref)
        dR = float(np.abs(R_mut - R_ref).max())
        print(f"{row['id']} without {drop[0]}.{drop[1]}: R relF x{mR[0] / aR[0]:.2f} max x{mR[1] / aR[1]:.2f} max|dR| {dR:.2e} relF {mR[0]:.2e} | "
              f"Y relF x{mY[0] / aY[0]:.2f} max x{mY[1] / aY[1]:.2f}")
        if row["facts"]["regime"] == "narrow" and drop in ig.MUTATIONS_R:
            assert dR > ig.R_BARS["narrow"][1], (drop, dR)

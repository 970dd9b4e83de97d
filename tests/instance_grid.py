"""The instance grid: one engine run per row, together launching every compiled instance of the iteration kernels.

TEST INFRASTRUCTURE (tests/test_instance_grid_cpu.py, tests/test_instance_grid_gpu.py).  The Harmony iteration is served
by a matrix of template instances picked at run time from the shape -- the cluster tiles mt = ceil(K / 16), the row
length dp, the one-hot tile count of the R^T.Z pass, the bf16 pipe or the f32-input form, the persistent or the
per-block sweep.  A row is `id, N, d, K, B, block_size, env, expect`: `expect` is the set of instances the row must
launch (the GPU test holds the library's launch census against it), stated by `dispatch()` below, which restates the
library's host-side selection predicates (hmx_capi.cpp round_body / blocks_loop / rtz3_pass / ridge_*, the launch_*
wrappers of hmx_kernels.hip and hmx_rtz3.hip) with the file and function each one comes from.  The rows are a covering
design -- every instance at least once -- not the cross product of the families.  UNREACHABLE lists the compiled
instances no shape and switch can select, each with the predicate that excludes it; the CPU test asserts that rows and
UNREACHABLE together are exactly the instances of FAMILIES in the built library.

Sizes are the smallest at which the hand-off between workgroups is real: narrow rows have N = 400 x (update blocks)
cells in B = 2 batches -- about 25 tiles per block, and under the group-affine map the larger batch (about 240 cells of a
block) gets two workgroups (plan_ga: ceil((240 + 5 sqrt 240) / 16) + 1 = 21 tiles > 14 per workgroup), so a count field
has two contributors; wide rows have N = 600 x (update blocks) cells in B = 3 batches, >= 33 tiles per block, so
k_sweep_wide3 has more than one 16-tile chunk per block.
"""
import re

# kernel families of the iteration (the LISI, kNN, I/O and scoring kernels are not part of this grid)
FAMILIES = ["k_round", "k_rtz3c", "k_rtz3", "k_rtz2", "k_assign_lds", "k_assign_wide", "k_assign_wide3", "k_sweep_wide3",
            "k_rtzw", "k_rtzw2b", "k_rtz_wide", "k_ridge_apply2", "k_ridge_apply_wide", "k_ridge_apply_wideb", "k_assign",
            "k_ridge_apply", "k_rtz", "k_kmeans_step"]
# k_kmeans_step<1..7> is launched by the device Lloyd, not by a round: tests/test_parity_gpu.py
# test_device_lloyd_matches_numpy_lloyd runs K = 12, 24, 40, 56, 72, 88, 100 and asserts the census there
LLOYD_INSTANCES = {f"k_kmeans_step<{m}>" for m in range(1, 8)}


# every engine switch a row may set (read per engine by read_switches(), hmx_capi.cpp): cleared before a row sets its own
SWITCHES = ["HMX_ROUND_MODE", "HMX_ROUND_F32", "HMX_ROUND_GA", "HMX_RTZ3_BF16", "HMX_RTZW_ZF", "HMX_WIDE_SWEEP", "HMX_RTZ", "HMX_FUSE_TABLE",
            "HMX_ROUND_WGS", "HMX_ROUND_REQ", "HMX_RTZ3_TASK_CAP", "HMX_TEST_FAIL_SWEEP", "HMX_SPIN_LIMIT", "HMX_CLUSTER_LOOP"]

# Bars of tests/test_instance_grid_gpu.py against float64; how they were chosen, r_max and s_min: profiles/instance_grid_errors.txt.
# factor x the row's anchor error for (relative Frobenius, max-abs / max |ref|), per regime: 1.25 x the largest engine / anchor
# ratio of two runs of the whole grid, rounded up (the generic last-resort kernels accumulate the ridge statistics
# in fp32 over long runs of tiles and sit further from the fp32 anchor than the others: they get their own factor instead of
# loosening everyone's)
BAR_FACTORS = {"Z_corr": {"narrow": (3.8, 4.0), "wide": (3.3, 3.1), "generic": (12.0, 10.8)},
               "Z_cos": {"narrow": (2.1, 2.0), "wide": (2.2, 2.3), "generic": (7.7, 7.2)},
               "Y": {"narrow": (1.3, None), "wide": (1.3, None), "generic": (1.3, None)}}
# R and Y: no factor separates the engine from a single dropped product (see the profile), so they keep the absolute bars of the
# direct A/B tests (tests/test_parity_gpu.py), here against float64: R (relative Frobenius, max |dR|) -- 6e-6 on max |dR| is the
# bar of k_round's A/B (rows of d <= 64 floats), 3e-5 and 6e-6 relative Frobenius those of the wide A/B (an R entry moves by
# c = 2 log2(e) / sigma = 28.9 times the rounding of a dot product of d terms: d up to 208 there); the generic rows (K = 250,
# d = 250: longer dot products and sums than any narrow row) go with the wide bars.  Y: max |dY| 2e-6 (the wide A/B), and
# since the engine's Y sits AT its anchor (r_max 0.98 in relative Frobenius) the factor above on that measure as well (the max measure is
# one element of d x K and moved by a quarter between two runs: 1.11 -> 1.39 on the narrow rows; it keeps the absolute bar alone).
R_BARS = {"narrow": (6e-6, 6e-6), "wide": (6e-6, 3e-5), "generic": (6e-6, 3e-5)}
Y_BAR = 2e-6
# the single dropped products (centroid term, cell term) whose error in R must exceed the narrow rows' bar on max |dR| (CPU test)
MUTATIONS_R = [("l", "h"), ("m", "m")]


def instance_name(mangled):
    """'_Z7k_roundILi5ELi16ELb1EEv9RoundArgs' -> 'k_round<5,16,true>' (Itanium names with integral template arguments;
    a plain kernel gives its name, anything else None)."""
    m = re.match(r"^_Z(\d+)", mangled)
    if not m:
        return None
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    if not rest.startswith("I"):
        return name
    args = []
    pos = 1
    while not rest.startswith("E", pos):
        a = re.match(r"L([ib])(n?\d+)E", rest[pos:])
        if not a:
            return None
        args.append(("true" if a.group(2) != "0" else "false") if a.group(1) == "b" else a.group(2).replace("n", "-"))
        pos += a.end()
    return f"{name}<{','.join(args)}>"


def family(instance):
    return instance.split("<")[0]


# ---- the library's shape arithmetic (hmx_capi.cpp hmx_create) ----------------------------------------------------
def row_floats(d):                       # hmx_kernels.hip round_row_floats, hmx_create
    return 32 if d <= 32 else 52 if d <= 52 else 64 if d <= 64 else (d + 15) & ~15


def n_blocks(block_size):                # harmony.py:474
    import math
    return int(math.ceil(1.0 / block_size))


def block_size_for(nblk):
    """a block size with ceil(1 / block_size) == nblk whose last block is shorter than the others"""
    return 1.0 / (nblk - 0.5)


def rtz3_ntb(dp, nblk):                  # hmx_rtz3.hip
    return max(0, (nblk - (64 - dp) + 15) // 16)


def rtz3_ok(mt, dp, nblk):               # hmx_rtz3.hip (G <= 64 holds for every row)
    return 1 <= mt <= 7 and dp in (32, 52, 64) and rtz3_ntb(dp, nblk) <= 2 and nblk <= 64


def rtz3b_ok(mt, dp, nblk, Kp):          # hmx_rtz3.hip: rtz3b_lds_bytes = 4 * RTZ3_WAVES (4) * (16 (Kp + dp) + 4) floats
    lds = 4 * 4 * (16 * (Kp + dp) + 4) * 4
    slab = mt * (4 + rtz3_ntb(dp, nblk)) * 256 * 4
    return rtz3_ntb(dp, nblk) <= 1 and max(lds, slab) <= 160 * 1024


def rtz_wide_ok(mt, dp):                 # hmx_kernels.hip
    return 1 <= mt <= 13 and dp % 16 == 0 and dp <= 208 and (mt > 7 or dp > 64)


def rtz2_ok(mt, dp):                     # hmx_kernels.hip
    return 1 <= mt <= 7 and dp in (32, 52, 64)


def rtzw_nt(dp, d, nblk):                # hmx_rtz3.hip
    return dp // 16 + max(0, (nblk - (dp - d) + 15) // 16)


def rtzw_ok(mt, dp, d, nblk):            # hmx_rtz3.hip (the G term holds for every row)
    return rtz_wide_ok(mt, dp) and rtzw_nt(dp, d, nblk) <= 16 and nblk <= 64


def rtzw2b_ok(mt, dp, d, nblk):          # hmx_rtz3.hip (its LDS term holds for every mt <= 13, dp <= 208)
    return rtzw_ok(mt, dp, d, nblk) and 8 <= mt <= 13 and 4 <= (rtzw_nt(dp, d, nblk) + 1) // 2 <= 7


def dispatch(d, K, nblk, env):
    """(instances one init_cluster + two rounds + two ridge steps launch, facts) for a single engine with one batch
    variable on the device update order.  `facts`: regime ('narrow' / 'wide' / 'generic'), bf16 (sweep on the bf16
    pipe), rtz_bf16 (round pass on it), ga (group-affine map), persistent (one launch per sweep)."""
    sw = lambda name, unset: int(env.get(name, unset))
    blocks_mode = env.get("HMX_ROUND_MODE") == "blocks"
    round_bf16, rtz_bf16 = not sw("HMX_ROUND_F32", 0), bool(sw("HMX_RTZ3_BF16", 1))
    zcf, wide_sweep, rtz_kernel = bool(sw("HMX_RTZW_ZF", 1)), bool(sw("HMX_WIDE_SWEEP", 1)), 2 if sw("HMX_RTZ", 3) == 2 else 3
    dp, mt, Kp = row_floats(d), (K + 15) // 16, (K + 3) & ~3
    ks, ntd = dp // 4, (dp + 15) // 16
    T = lambda b: "true" if b else "false"
    out = set()
    facts = dict(bf16=False, rtz_bf16=False, ga=False, persistent=False, presplit=False)
    narrow, wide = mt <= 7 and dp <= 64, rtz_wide_ok(mt, dp)
    facts["regime"] = "narrow" if narrow else "wide" if wide else "generic"
    use_rtz3 = rtz_kernel == 3 and narrow and rtz3_ok(mt, dp, nblk)          # hmx_capi.cpp use_rtz3 / use_rtzw
    use_rtzw = rtz_kernel == 3 and wide and rtzw_ok(mt, dp, d, nblk)
    quad = 8 if (rtz_bf16 and rtz3b_ok(mt, dp, nblk, Kp)) else 4              # hmx_rtz3.hip rtz3_quad (cut once, at upload)

    def streaming_pass(cols, ridge):                                          # hmx_capi.cpp rtz3_pass, launch_rtz3 / launch_rtzw
        if use_rtz3 and rtz3_ok(mt, dp, cols):
            ntb = rtz3_ntb(dp, cols)
            if rtz_bf16 and quad == 8 and rtz3b_ok(mt, dp, cols, Kp):
                out.add(f"k_rtz3c<{mt},{ks},{ntb}>")
                return True
            assert quad == 4, "tasks cut for eight waves cannot run k_rtz3"
            out.add(f"k_rtz3<{mt},{ks},{ntb}>")
            return False
        if rtz_bf16 and rtzw2b_ok(mt, dp, d, cols):
            zf = not ridge and zcf                                            # the ridge statistics run on Z_orig: no planes
            out.add(f"k_rtzw2b<{mt},{(rtzw_nt(dp, d, cols) + 1) // 2},{T(zf)}>")
            facts["presplit"] = facts["presplit"] or zf
            return True
        out.add(f"k_rtzw<{mt}>")
        return False

    def list_order_pass(in_round):                                            # round_body / centroid_pass / ridge_stats without the streaming pass
        if rtz2_ok(mt, dp) and not (in_round and blocks_mode):
            out.add(f"k_rtz2<{mt},{2 if dp == 32 else 4},{T(dp == 52)}>")     # launch_rtz2: a padding column carries the sums at dp = 52
        elif wide:
            out.add(f"k_rtz_wide<{mt}>")
        else:
            out.add("k_rtz<7,4>")

    def assign(penalty, bf16_frags):                                          # hmx_kernels.hip launch_assign
        if narrow:
            out.add(f"k_assign_lds<{mt},{T(penalty)}>")
        elif wide:
            if penalty and bf16_frags:
                out.add(f"k_assign_wide3<{mt}>")
                return True
            out.add(f"k_assign_wide<{mt},{T(penalty)}>")
        else:
            out.add(f"k_assign<{7 if mt <= 7 else 13 if mt <= 13 else 20},{2 if mt <= 7 else 1},{T(penalty)}>")
        return False

    assign(False, False)                                                      # hmx_init_cluster
    # ---- a round (round_body)
    persistent = not blocks_mode
    mega = persistent and narrow                                              # (k_round's LDS bound holds at two batches)
    facts["persistent"] = mega
    facts["ga"] = mega and bool(sw("HMX_ROUND_GA", 1))
    if use_rtz3 or use_rtzw:
        facts["rtz_bf16"] = streaming_pass(nblk, False)
    else:
        list_order_pass(True)
    if mega:                                                                  # launch_round (round_uses_bf16_pipe: fits at two batches)
        out.add(f"k_round<{mt},{ks},{T(round_bf16)}>")
        facts["bf16"] = round_bf16
    else:                                                                     # blocks_loop
        y_frags = round_bf16 and wide
        if y_frags and wide_sweep:         # wide_sweep_planned (single engine, lists with run offsets)
            out.add(f"k_sweep_wide3<{mt}>")
            facts["bf16"] = facts["persistent"] = True
        else:
            facts["bf16"] = assign(True, y_frags)
    # ---- the ridge (ridge_stats, ridge_solve_apply, launch_ridge_apply)
    if use_rtz3 or use_rtzw:
        streaming_pass(1, True)
    else:
        list_order_pass(False)
    if wide:
        out.add(f"k_ridge_apply_wide{'b' if round_bf16 else ''}<{dp // 16}>")
    elif rtz2_ok(mt, dp):
        out.add(f"k_ridge_apply2<{2 if dp == 32 else 4},{mt}>")
    else:
        out.add(f"k_ridge_apply<{4 if ntd <= 4 else 13 if ntd <= 13 else 20},{2 if ntd <= 13 else 1}>")
    return out, facts


# ---- the compiled instances no shape and switch can select -------------------------------------------------------
UNREACHABLE = {}
for _mt in range(1, 8):
    for _k in ("k_rtz3c", "k_rtz3"):
        UNREACHABLE[f"{_k}<{_mt},16,0>"] = ("rtz3_ntb(dp, nblk) = max(0, (nblk - (64 - dp) + 15) / 16) (hmx_rtz3.hip): KS = 16 is dp = 64, no "
                                            "padding column, so ntb >= 1 for every nblk >= 1")
UNREACHABLE["k_rtz3c<7,16,1>"] = ("rtz3b_ok (hmx_rtz3.hip): rtz3b_lds_bytes(Kp, dp) = 64 (16 (Kp + dp) + 4) <= 160 KB needs Kp + dp <= 159; "
                                  "MT = 7 has Kp >= 100 and KS = 16 has dp = 64")
for _k in ("k_ridge_apply_wide", "k_ridge_apply_wideb"):
    UNREACHABLE[f"{_k}<1>"] = ("launch_ridge_apply (hmx_kernels.hip): MTD = dp / 16 under rtz_wide_ok(mt, dp); hmx_create pads rows to "
                               "round_row_floats(d) = 32, 52, 64 or the next multiple of 16 above 64, never to 16")
    UNREACHABLE[f"{_k}<3>"] = ("launch_ridge_apply (hmx_kernels.hip): MTD = dp / 16 under rtz_wide_ok(mt, dp), which needs dp % 16 == 0; "
                               "33 <= d <= 52 is padded to dp = 52 (round_row_floats), never to 48")


# ---- the rows ---------------------------------------------------------------------------------------------------
F32 = {"HMX_ROUND_F32": "1", "HMX_RTZ3_BF16": "0"}
ROWS = []


def _row(tag, d, K, nblk, env=None, per_block=None):
    env = dict(env or {})
    mt, dp = (K + 15) // 16, row_floats(d)
    expect, facts = dispatch(d, K, nblk, env)
    wide = facts["regime"] != "narrow"
    per_block = per_block or (600 if wide else 400)
    ROWS.append(dict(id=f"{tag}-mt{mt}-dp{dp}-d{d}-K{K}-b{nblk}" + "".join(f"-{k[4:]}={v}" for k, v in sorted(env.items())),
                     N=per_block * nblk, d=d, K=K, B=3 if wide else 2, block_size=block_size_for(nblk), nblk=nblk, env=env,
                     expect=frozenset(expect), facts=facts))


def _narrow_K(mt, dp):
    """K off the tile size (16 mt - 3) where k_rtz3c's LDS bound Kp + dp <= 159 (rtz3b_ok) allows it: at mt = 6, dp = 64 it
    needs K <= 92 (K = 93 rounds to Kp = 96: 160) and at mt = 7, dp = 52 K <= 104, so those pairs take K = 91 and K = 103"""
    return {(6, 64): 91, (7, 52): 103}.get((mt, dp), 16 * mt - 3)


_D = {32: 29, 52: 47, 64: 61}                                  # d off the row size
# block counts that hit each reachable one-hot tile count of the R^T.Z pass (rtz3_ntb): 0 / 1 / 2
_BLOCKS = {32: (20, 40, 60), 52: (10, 20, 40), 64: (16, 20)}
for _mt in range(1, 8):                                         # narrow, default switches: k_rtz3c (k_rtz3 where ntb = 2), k_round<..,true>,
    for _dp in (32, 52, 64):                                    # k_assign_lds<..,false>, k_ridge_apply2
        for _nb in _BLOCKS[_dp]:
            _row("narrow", _D[_dp], _narrow_K(_mt, _dp), _nb)
for _d, _K, _nb in ((32, 48, 20), (52, 80, 20), (64, 112, 16)):  # d = dp exactly and K = 16 mt exactly
    _row("narrow-exact", _d, _K, _nb)
for _mt in range(1, 8):                                         # the f32-input forms: k_round<..,false>, k_rtz3 (the ridge pass adds ntb(1))
    for _dp in (32, 52, 64):
        for _nb in _BLOCKS[_dp][1:] if _dp != 64 else (20,):
            _row("narrow-f32", _D[_dp], _narrow_K(_mt, _dp), _nb, F32)
for _i, _mt in enumerate(range(1, 8)):                          # a diagonal under three more settings
    _dp = (32, 52, 64)[_i % 3]
    _row("narrow-classic-map", _D[_dp], _narrow_K(_mt, _dp), 20 if _dp != 64 else 16, {"HMX_ROUND_GA": "0"})
for _mt in range(1, 8):
    _dp = (32, 52, 64)[_mt % 3]
    _row("narrow-blocks", _D[_dp], _narrow_K(_mt, _dp), 20 if _dp != 64 else 16, {"HMX_ROUND_MODE": "blocks"})   # k_assign_lds<..,true>
for _mt in range(1, 8):
    for _dp in (32, 52, 64):
        _row("narrow-rtz2", _D[_dp], _narrow_K(_mt, _dp), 20, {"HMX_RTZ": "2"})                                 # k_rtz2<MT, NTD, ONES>

# wide, default switches.  d = 16 t - 3 has dp / 16 = t column tiles and, at 20 blocks, rtzw_nt = t + 2.
_WIDE_D = {1: 77, 2: 93, 3: 109, 4: 125, 5: 141, 6: 157, 7: 173, 8: 189, 9: 205, 10: 29, 11: 61, 12: 77, 13: 93}   # mt -> d: every dp / 16 in {2, 4, 5..13}
for _mt in range(1, 14):                                        # k_sweep_wide3, k_assign_wide<..,false>, k_ridge_apply_wideb, k_rtzw / k_rtzw2b
    _row("wide", _WIDE_D[_mt], 16 * _mt - 3, 20)
for _mt in range(8, 14):                                        # k_rtzw2b<MT, NTH, true>: NTH = (rtzw_nt + 1) / 2 = 4..7
    _row("wide-nth4", 61, 16 * _mt - 3, 40)                     # dp = 64, 40 blocks: nt = 4 + 3
    for _t, _nb in ((7, 20), (10, 20), (12, 20)):               # nt = t + 2 = 9, 12, 14: NTH = 5, 6, 7
        _row(f"wide-nth{(_t + 3) // 2}", 16 * _t - 3, 16 * _mt - 3, _nb)
_row("wide-exact", 208, 208, 20)                                # d = dp and K = 16 mt exactly
for _mt in range(1, 14):                                        # the switches of the wide A/B test, and HMX_RTZ=2
    _row("wide-blocks", _WIDE_D[_mt], 16 * _mt - 3, 20, {"HMX_WIDE_SWEEP": "0"})      # k_assign_wide3
    _row("wide-f32", _WIDE_D[_mt], 16 * _mt - 3, 20, {"HMX_ROUND_F32": "1"})           # k_assign_wide<..,true>, k_ridge_apply_wide
    _row("wide-rtz2", _WIDE_D[_mt], 16 * _mt - 3, 20, {"HMX_RTZ": "2"})                # k_rtz_wide
for _mt in range(8, 14):
    _row("wide-rtz-f32", _WIDE_D[_mt], 16 * _mt - 3, 20, {"HMX_RTZ3_BF16": "0"})       # k_rtzw<8..13>
    for _t, _nb, _d in ((4, 40, 61), (7, 20, 109), (10, 20, 157), (12, 20, 189)):     # k_rtzw2b<MT, NTH, false> at NTH = 4..7
        _row(f"wide-zf0-nth{(rtzw_nt(16 * _t, _d, _nb) + 1) // 2}", _d, 16 * _mt - 3, _nb, {"HMX_RTZW_ZF": "0"})

# the generic kernels: K > 112 with 33..52 PCs (rows of 52 floats are no whole 16-column steps); K or d in 209..320
_row("generic", 40, 150, 20, per_block=400)                     # k_assign<13,1,*>, k_ridge_apply<4,2>, k_rtz<7,4>
_row("generic", 100, 250, 20, per_block=400)                    # k_assign<20,1,*>, k_ridge_apply<13,2>
_row("generic", 250, 30, 20, per_block=400)                     # k_assign<7,2,*>, k_ridge_apply<20,1>

assert len({r["id"] for r in ROWS}) == len(ROWS)


def covered():
    s = set(LLOYD_INSTANCES)
    for r in ROWS:
        s |= r["expect"]
    return s

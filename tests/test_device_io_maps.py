"""CPU replay of the index maps of the device I/O kernels (harmonypy_amd/csrc/hmx_io.hip), in the style of
test_rtz3_maps.py: every workgroup's loops evaluated with NumPy over flat buffers, so that bounds, padding, ragged
last slabs, strided and sliced sources and the inverse cell map are checked without a GPU.  Also: host data (NumPy,
CPU tensors) keeps the NumPy path of run_harmony."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT

SRC = open(os.path.join(ROOT, "harmonypy_amd", "csrc", "hmx_io.hip")).read()
IO_THREADS = int(re.search(r"constexpr int IO_THREADS = (\d+);", SRC).group(1))
IO_ROWS = int(re.search(r"constexpr int IO_ROWS = (\d+);", SRC).group(1))


def io_slab(cols):
    """io_slab(): odd pitch, 2^lg_s cells, tile within 64 KB."""
    pitch = cols | 1
    lg_s = 7 if pitch * 128 * 4 <= 65536 else 6 if pitch * 64 * 4 <= 65536 else 5
    return pitch, lg_s


def uses_slab(s_cell, s_feat):
    return s_cell == 1 and s_feat != 1


def load(src, s_cell, s_pc, cmap, d, dp, N):
    """launch_io_load: returns (dst N x dp, write count per element)."""
    dst = np.full(N * dp, np.nan, np.float32)
    hits = np.zeros(N * dp, np.int64)
    if uses_slab(s_cell, s_pc):
        inv = None if cmap is None else np.empty(N, np.int64)
        if cmap is not None:
            inv[cmap] = np.arange(N)                                       # k_io_invert
        pitch, lg = io_slab(d)
        S = 1 << lg
        assert (S * pitch * 4) <= 65536
        for b in range(-(-N // S)):
            n0, tile = b * S, np.full(S * pitch, np.nan, np.float32)
            ns = min(S, N - n0)
            i = np.arange(d << lg)
            f, j = i >> lg, i & (S - 1)
            m = j < ns
            a = f[m] * s_pc + n0 + j[m]
            assert a.min() >= 0 and a.max() < src.size
            t = j[m] * pitch + f[m]
            assert t.max() < S * pitch
            tile[t] = src[a]
            i = np.arange(ns * dp)
            j, c = i // dp, i % dp
            r = n0 + j if inv is None else inv[n0 + j]
            o = r * dp + c
            assert o.min() >= 0 and o.max() < N * dp
            v = np.where(c < d, tile[j * pitch + np.minimum(c, d - 1)], 0.0)
            assert not np.isnan(v).any(), "a tile element was read before it was written"
            dst[o] = v
            np.add.at(hits, o, 1)
        return dst.reshape(N, dp), hits
    for b in range(-(-N // IO_ROWS)):
        r0 = b * IO_ROWS
        i = np.arange(min(IO_ROWS, N - r0) * dp)
        j, c = i // dp, i % dp
        r = r0 + j
        sr = r if cmap is None else cmap[r]
        a = sr * s_cell + np.minimum(c, d - 1) * s_pc
        assert a.min() >= 0 and a.max() < src.size
        dst[r0 * dp + i] = np.where(c < d, src[a], 0.0)
        np.add.at(hits, r0 * dp + i, 1)
    return dst.reshape(N, dp), hits


def store(eng, ld, cols, cmap, dst, s_cell, s_col, N):
    """launch_io_store into the flat buffer dst; returns the write count per element of dst."""
    hits = np.zeros(dst.size, np.int64)
    src = eng.reshape(-1)
    if uses_slab(s_cell, s_col):
        inv = None if cmap is None else np.empty(N, np.int64)
        if cmap is not None:
            inv[cmap] = np.arange(N)
        pitch, lg = io_slab(cols)
        S = 1 << lg
        for b in range(-(-N // S)):
            n0, tile = b * S, np.full(S * pitch, np.nan, np.float32)
            ns = min(S, N - n0)
            i = np.arange(ns * cols)
            j, c = i // cols, i % cols
            r = n0 + j if inv is None else inv[n0 + j]
            tile[j * pitch + c] = src[r * ld + c]
            i = np.arange(cols << lg)
            f, j = i >> lg, i & (S - 1)
            m = j < ns
            o = f[m] * s_col + n0 + j[m]
            assert o.min() >= 0 and o.max() < dst.size
            v = tile[j[m] * pitch + f[m]]
            assert not np.isnan(v).any()
            dst[o] = v
            np.add.at(hits, o, 1)
        return hits
    for b in range(-(-N // IO_ROWS)):
        r0 = b * IO_ROWS
        i = np.arange(min(IO_ROWS, N - r0) * cols)
        j, c = i // cols, i % cols
        r = r0 + j
        dr = r if cmap is None else cmap[r]
        o = dr * s_cell + c * s_col
        assert o.min() >= 0 and o.max() < dst.size
        dst[o] = src[r * ld + c]
        np.add.at(hits, o, 1)
    return hits


def _views(Z, rng):
    """(name, flat buffer, stride_cell, stride_feature) holding the N x d matrix Z in several layouts."""
    N, d = Z.shape
    out = [("nxd", Z.reshape(-1).copy(), d, 1), ("dxn", Z.T.reshape(-1).copy(), 1, N)]
    wide = rng.normal(size=(N, d + 14)).astype(np.float32)              # [:, 3:3+d] of a wider matrix
    wide[:, 3:3 + d] = Z
    out.append(("col_slice", wide.reshape(-1)[3:], d + 14, 1))
    tall = rng.normal(size=(d + 5, N)).astype(np.float32)               # rows 2..2+d of a taller d x N matrix, transposed
    tall[2:2 + d] = Z.T
    out.append(("t_of_slice", tall.reshape(-1)[2 * N:], 1, N))
    sparse = rng.normal(size=(N, 2 * d)).astype(np.float32)             # every other column: no stride of 1
    sparse[:, ::2] = Z
    out.append(("strided", sparse.reshape(-1), 2 * d, 2))
    return out


def _perm(N, G, rng):
    """A group-sorted cell map as build_layout makes it: internal row -> caller row."""
    g = rng.integers(0, G, size=N)
    return np.argsort(g, kind="stable").astype(np.int64)


@pytest.mark.parametrize("N,d,dp", [(1000, 50, 52), (130, 20, 32), (257, 200, 208), (77, 320, 320), (64, 7, 16), (1, 3, 16)])
@pytest.mark.parametrize("mapped", [True, False])
def test_load_maps_every_layout_into_padded_group_sorted_rows(N, d, dp, mapped):
    rng = np.random.default_rng(N + d)
    Z = rng.normal(size=(N, d)).astype(np.float32)
    cmap = _perm(N, 5, rng) if mapped else None
    want = np.zeros((N, dp), np.float32)
    want[:, :d] = Z if cmap is None else Z[cmap]
    for name, flat, sc, sp in _views(Z, rng):
        got, hits = load(flat, sc, sp, cmap, d, dp, N)
        assert (hits == 1).all(), name                                  # every element of N x dp written once
        np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("N,cols,ld", [(1000, 50, 52), (300, 37, 40), (129, 200, 208), (70, 320, 320), (1, 5, 8)])
@pytest.mark.parametrize("mapped", [True, False])
def test_store_writes_the_view_and_nothing_else(N, cols, ld, mapped):
    rng = np.random.default_rng(N * cols)
    eng = rng.normal(size=(N, ld)).astype(np.float32)                   # internal rows (padding columns included)
    cmap = _perm(N, 7, rng) if mapped else None
    want = np.empty((N, cols), np.float32)
    if cmap is None:
        want[:] = eng[:, :cols]
    else:
        want[cmap] = eng[:, :cols]                                      # caller row cmap[r] <- internal row r
    layouts = [("nxd", N * cols, cols, 1, lambda b: b.reshape(N, cols)),
               ("dxn", N * cols, 1, N, lambda b: b.reshape(cols, N).T),
               ("col_slice", N * (cols + 9), cols + 9, 1, lambda b: b.reshape(N, cols + 9)[:, 4:4 + cols]),
               ("t_of_slice", (cols + 5) * N, 1, N, lambda b: b.reshape(cols + 5, N)[2:2 + cols].T),
               ("strided", N * 2 * cols, 2 * cols, 2, lambda b: b.reshape(N, 2 * cols)[:, ::2])]
    for name, size, sc, scol, view in layouts:
        buf = np.full(size, 7.5, np.float32)
        off = {"col_slice": 4, "t_of_slice": 2 * N}.get(name, 0)
        sub = buf[off:]
        hits = store(eng, ld, cols, cmap, sub, sc, scol, N)
        np.testing.assert_array_equal(view(buf), want, err_msg=name)
        written = np.zeros(size, bool)
        written[off:] = hits > 0
        assert hits.max() == 1, name                                    # no element written twice
        assert written.sum() == N * cols, name                          # only the view's elements
        assert (buf[~written] == 7.5).all(), name


@pytest.mark.parametrize("cols", [1, 2, 20, 50, 64, 127, 128, 200, 255, 256, 320])
def test_slab_tile_fits_and_its_column_accesses_do_not_conflict(cols):
    """The tile stays within 64 KB; the column accesses of a wave (lane = cell j, address j * pitch + f, ds_write_b32 /
    ds_read_b32: 32 banks, lanes in two 32-lane halves) fall on 32 distinct banks."""
    pitch, lg = io_slab(cols)
    S = 1 << lg
    assert pitch % 2 == 1 and pitch >= cols and S * pitch * 4 <= 65536 and S >= 32
    for f in (0, cols - 1):
        for half in range(0, min(S, 64), 32):
            lanes = np.arange(half, half + 32) % S
            banks = (lanes * pitch + f) % 32
            assert len(set(banks.tolist())) == 32


def test_kernels_take_the_coalesced_path_per_orientation():
    assert not uses_slab(50, 1)            # row-major: whole rows
    assert uses_slab(1, 1000)              # d x N, .T of row-major: LDS slab
    assert not uses_slab(100, 2)           # neither stride 1: element-wise
    assert not uses_slab(1, 1)             # a single feature or a single cell


def test_host_data_keeps_the_numpy_path():
    import torch
    from harmonypy_amd.harmony import _as_device_tensor, _prepare_inputs
    rng = np.random.default_rng(0)
    Z = rng.normal(size=(60, 6)).astype(np.float32)
    meta = pd.DataFrame({"b": ["x", "y", "z"] * 20})
    for x in (Z, torch.from_numpy(Z), torch.from_numpy(Z.astype(np.float64)), torch.from_numpy(Z).T):
        assert _as_device_tensor(x) is None
        p = _prepare_inputs(x, meta, "b")
        assert isinstance(p["Z"], np.ndarray) and p["Z"].dtype == np.float32 and not p["on_device"]
        np.testing.assert_array_equal(p["Z"], Z.T)


def test_device_io_symbols_are_declared_and_exported():
    """include/hmx_device_io.h declares what the binding lists as DEVICE_IO_EXPORTS; the library exports them; hmx.h
    itself is unchanged in what it declares."""
    from harmonypy_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "hmx_device_io.h")).read()
    declared = sorted(set(re.findall(r"\b(hmx_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(_capi.DEVICE_IO_EXPORTS)
    assert not set(declared) & set(_capi.EXPORTS)
    if os.path.exists(_capi.LIB_PATH):
        lib = _capi.load()
        for name in declared:
            assert hasattr(lib, name), name

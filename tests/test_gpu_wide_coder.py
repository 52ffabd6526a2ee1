"""GPU: the windowed factorized coder (``lla_quantise_encode_wide``, ``lla_rans_decode_batch_wide``,
``lla_rans_decode_gather_wide``) against the library's host coder, which has no size limit.  Everything is exact: bytes,
lengths, symbols, fp32 bits, statuses.  ``window_channels`` puts window borders inside tiny shapes; the two large shapes
are ones the resident kernels refuse."""
import functools

import numpy as np
import pytest
import torch

from wide_coder_util import (P, dev_tables, device_decode_wide, device_encode, device_gather_wide, host_dequantise,
                             host_encode, in_table_symbols, make_tables, padded, plant_escapes, z_for)

pytestmark = pytest.mark.gpu

ENCODE, DECODE, GATHER = 0, 1, 2
SMALL = (37, 9)                       # C % 4 = 1: channel 36 is encode_walk's tail
# first / last channel of windows of 4, 8 and 36 channels, and the C % 4 tail
EDGE_CHANNELS = (0, 3, 4, 7, 8, 31, 32, 35, 36)


def _lib():
    from lossyless_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def small_case(B, seed=3):
    """C = 37, W = 9: fp32 z with escapes on the window edges, its symbols, and the host coder's streams."""
    C, W = SMALL
    tab = make_tables(C, W, seed=11)
    z = z_for(plant_escapes(in_table_symbols(tab, B, seed), tab, EDGE_CHANNELS), tab)
    return tab, z


def _quantise(z, d):
    L = _lib()
    zt = torch.from_numpy(z).cuda()
    sym = torch.empty(zt.shape, dtype=torch.int32, device="cuda")
    L.check(L.lib().lla_quantise(L.ptr(zt), L.LLA_Z_F16 if zt.dtype == torch.float16 else L.LLA_Z_F32, zt.shape[0],
                                 zt.shape[1], L.ptr(d["bias"]), L.ptr(d["exp_scale"]), L.ptr(d["median"]), L.ptr(sym),
                                 L.stream_ptr()), "lla_quantise")
    return sym.cpu().numpy()


@functools.lru_cache(maxsize=None)
def small_reference(B, half):
    """-> (tables, device tables, z as coded, lla_quantise's symbols, host streams, host offsets, resident streams)."""
    tab, z = small_case(B)
    z = z.astype(np.float16) if half else z
    d = dev_tables(tab)
    sym = _quantise(z, d)
    pay, off = host_encode(sym, tab)
    rc, res, res_len, _ = device_encode(z, d, SMALL[1])
    assert rc == 0
    return tab, d, z, sym, pay, off, (res, res_len)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("window", [4, 8, 36, 40, 0])
def test_window_edges_encode(window, half):
    tab, d, z, sym, pay, off, (res, res_len) = small_reference(70, half)
    esc = (sym < tab["offset"]) | (sym >= tab["offset"] + tab["cdf_len"] - 2)
    assert all(esc[:, c].any() for c in EDGE_CHANNELS)              # escapes where the windows meet and in the tail
    rc, s, ln, sym_out = device_encode(z, d, SMALL[1], window=window, want_symbols=True)
    assert rc == 0
    assert np.array_equal(sym_out, sym)                             # the fused form's symbols_out == lla_quantise
    assert np.array_equal(ln, np.diff(off.astype(np.int64))) and np.array_equal(s, pay)     # == the host coder
    assert np.array_equal(ln, res_len) and np.array_equal(s, res)                           # == lla_quantise_encode


@pytest.mark.parametrize("window", [4, 8, 36, 40, 0])
def test_window_edges_symbols_mode_decode_and_gather(window):
    """Symbols in (huge escapes included) == lla_rans_encode_batch == host; both decoders give them back."""
    C, W = SMALL
    tab, d, _, sym, _, _, _ = small_reference(70, False)
    sym = sym.copy()
    sym[0], sym[1] = -2 ** 29, 2 ** 29                              # every channel escaped with 8 payload digits
    sym[2] = tab["offset"] + tab["cdf_len"] - 2                     # exactly the escape index
    pay, off = host_encode(sym, tab)
    rc, s, ln, copy = device_encode(sym, d, W, window=window, want_symbols=True)
    assert rc == 0 and np.array_equal(copy, sym)
    assert np.array_equal(ln, np.diff(off.astype(np.int64))) and np.array_equal(s, pay)
    rc, res, res_len, _ = device_encode(sym, d, W)
    assert rc == 0 and np.array_equal(res, pay) and np.array_equal(res_len, ln)
    rc, back, status = device_decode_wide(pay, off, 0, 70, d, C, W, window)
    assert rc == 0 and np.array_equal(back, sym) and not status.any()
    idx = np.random.default_rng(5).permutation(70)
    rc, out, status = device_gather_wide(pay, off, 0, 70, idx, d, C, W, window)
    assert rc == 0 and not status.any()
    assert np.array_equal(out.numpy().view(np.uint32), host_dequantise(sym[idx], tab).view(np.uint32))


def test_second_workgroup_with_one_live_lane():
    C, W = SMALL
    tab, d, z, sym, pay, off, _ = small_reference(257, False)
    rc, s, ln, sym_out = device_encode(z, d, W, window=8, want_symbols=True)
    assert rc == 0 and np.array_equal(sym_out, sym)
    assert np.array_equal(ln, np.diff(off.astype(np.int64))) and np.array_equal(s, pay)
    rc, back, status = device_decode_wide(pay, off, 0, 257, d, C, W, 8)
    assert rc == 0 and np.array_equal(back, sym) and not status.any()
    idx = np.arange(257)[::-1].copy()
    rc, out, status = device_gather_wide(pay, off, 0, 257, idx, d, C, W, 8)
    assert rc == 0 and not status.any()
    assert np.array_equal(out.numpy().view(np.uint32), host_dequantise(sym[idx], tab).view(np.uint32))


@pytest.mark.parametrize("C,W,B", [(1200, 40, 300), (2050, 33, 130)])
def test_shapes_the_resident_kernels_refuse(C, W, B):
    L = _lib().lib()
    assert [L.lla_rans_table_fits(C, W, k) for k in (ENCODE, DECODE, GATHER)] == [0, 0, 0]
    tab = make_tables(C, W, seed=C)
    d = dev_tables(tab)
    sym = plant_escapes(in_table_symbols(tab, B, 7), tab, (0, 15, 16, 111, 112, 113, C - 2, C - 1), magnitude=10 ** 6)
    assert device_encode(sym, d, W)[0] == -1                        # ... and the resident entry point says so itself
    pay, off = host_encode(sym, tab, prefix=1)
    rc, s, ln, _ = device_encode(sym, d, W, window=0)
    assert rc == 0 and np.array_equal(ln + 4, np.diff(off.astype(np.int64)))
    assert np.array_equal(s, host_encode(sym, tab)[0])
    # the fused form at this width: fp32 z -> the symbols lla_quantise gives -> the host coder's bytes
    z = z_for(np.clip(sym, -30000, 30000), tab)
    zsym = _quantise(z, d)
    rc, s, ln, sym_out = device_encode(z, d, W, window=0, want_symbols=True)
    assert rc == 0 and np.array_equal(sym_out, zsym) and np.array_equal(s, host_encode(zsym, tab)[0])
    rc, back, status = device_decode_wide(pay, off, 1, B, d, C, W, 0)
    assert rc == 0 and np.array_equal(back, sym) and not status.any()
    idx = np.random.default_rng(C).integers(0, B, size=B + 9)       # repeats
    want = host_dequantise(sym[idx], tab)
    rc, out, status = device_gather_wide(pay, off, 1, B, idx, d, C, W, 0)
    assert rc == 0 and not status.any()
    assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))
    rc, out16, status = device_gather_wide(pay, off, 1, B, idx, d, C, W, 0, dtype="float16")
    assert rc == 0 and not status.any()
    assert torch.equal(out16, out.half())                           # fp16 output == the fp32 output rounded


def _host_gather(pay, off, prefix, N, index, tab, ld, off_first=0, off_step=1):
    """The reference of the gather tests: lla_rans_decode_gather_host over the records the strided form names."""
    from latents_util import host_gather
    off = np.ascontiguousarray(off, dtype=np.uint64)
    if (off_first, off_step) != (0, 1):      # the host twin has no strided form: hand it the named records' offsets
        recs = off_first + np.arange(N) * off_step
        sub = [pay[int(off[r]):int(off[r + 1])] for r in recs]
        off = np.concatenate([[0], np.cumsum([len(s) for s in sub])]).astype(np.uint64)
        pay = np.concatenate(sub)
    return host_gather(padded(pay), off, prefix, index, tab, ld=ld, fill=-777.0)


@pytest.mark.parametrize("window", [8, 16, 0])
@pytest.mark.parametrize("prefix", [0, 1])
def test_gather_statuses_and_layout(window, prefix):
    """Repeats, indices outside [0, N), ld_out > C, a truncated and an unopenable record between healthy neighbours (the
    lanes without a record must stay with the workgroup: their neighbours' rows are complete)."""
    C, W = SMALL
    N = 70
    tab, d, _, sym, _, _, _ = small_reference(N, False)
    raw, roff = host_encode(sym, tab)
    strings = [raw[int(roff[i]):int(roff[i + 1])].tobytes() for i in range(N)]
    strings[20] = strings[20][:-8] if len(strings[20]) >= 16 else strings[20][:8]      # truncated: overruns while decoding
    strings[41] = strings[41][:4]                                                      # cannot be opened at all
    parts = [(len(s).to_bytes(4, "big") if prefix else b"") + s for s in strings]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    pay = np.frombuffer(b"".join(parts), np.uint8)
    index = np.array([5, 5, 19, 20, 21, -1, 40, 41, 42, N, 69, 0, 20, 2 ** 40], dtype=np.int64)
    ld = C + 3
    rc_h, want, st_h = _host_gather(pay, off, prefix, N, index, tab, ld)
    assert rc_h == 0
    assert st_h.tolist() == [0, 0, 0, 1, 0, 2, 0, 1, 0, 2, 0, 0, 1, 2]          # (what the reference says, spelled out)
    rc, out, status = device_gather_wide(pay, off, prefix, N, index, d, C, W, window, ld=ld)
    assert rc == 0 and status.tolist() == st_h.tolist()
    assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))    # bad rows zero, columns >= C untouched
    bad = status != 0
    assert not out.numpy()[bad, :C].any() and (out.numpy()[:, C:] == -777.0).all()
    assert np.array_equal(out.numpy()[~bad, :C].view(np.uint32), host_dequantise(sym[index[~bad]], tab).view(np.uint32))
    # the batch decoder on the same records: 20 overruns, 41 is a row of zeros, the rest are the symbols
    rc, back, st = device_decode_wide(pay, off, prefix, N, d, C, W, window)
    good = np.ones(N, bool)
    good[[20, 41]] = False
    assert rc == 0 and st[20] == 1 and st[41] == 1 and not st[good].any()
    assert np.array_equal(back[good], sym[good]) and not back[41].any()


def test_gather_and_decode_over_every_second_record():
    """off_first = 1, off_step = 2: the odd records of an interleaved body."""
    C, W = SMALL
    N = 70
    tab, d, _, sym, _, _, _ = small_reference(N, False)
    raw, roff = host_encode(sym, tab)
    filler = b"\x01\x02\x03\x04" * 3
    parts = []
    for i in range(N):
        s = raw[int(roff[i]):int(roff[i + 1])].tobytes()
        parts += [len(filler).to_bytes(4, "big") + filler, len(s).to_bytes(4, "big") + s]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    pay = np.frombuffer(b"".join(parts), np.uint8)
    index = np.array([3, 69, 0, 3, -5, N], dtype=np.int64)
    rc_h, want, st_h = _host_gather(pay, off, 1, N, index, tab, C, off_first=1, off_step=2)
    rc, out, status = device_gather_wide(pay, off, 1, N, index, d, C, W, 8, off_first=1, off_step=2)
    assert rc == 0 and rc_h == 0 and status.tolist() == st_h.tolist() == [0, 0, 0, 0, 2, 2]
    assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))
    rc, back, st = device_decode_wide(pay, off, 1, N, d, C, W, 8, off_first=1, off_step=2)
    assert rc == 0 and not st.any() and np.array_equal(back, sym)


def test_refusals():
    L, lib = _lib(), _lib().lib()
    C, W = SMALL
    tab, d, z, sym, pay, off, _ = small_reference(70, False)
    assert device_encode(z, d, W, window=6)[0] == L.LLA_EINVAL
    assert device_decode_wide(pay, off, 0, 70, d, C, W, 6)[0] == L.LLA_EINVAL
    assert device_gather_wide(pay, off, 0, 70, np.arange(4), d, C, W, 6)[0] == L.LLA_EINVAL
    assert device_encode(z, d, W, window=-4)[0] == L.LLA_EINVAL
    # a W whose smallest window (4 channels, two buffers) cannot fit: the bound include/lossyless_amd.h states
    wmax = 3000
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "lossyless_amd.h")).read()
    assert f"#define LLA_WIDE_MAX_W {wmax}\n" in header
    for kind in (ENCODE, DECODE, GATHER):
        assert lib.lla_rans_wide_window(8, wmax, kind, 0, None) == 4
        assert lib.lla_rans_wide_window(8, wmax + 1, kind, 0, None) == L.LLA_EINVAL
        assert lib.lla_rans_wide_window(8, wmax, kind, 8, None) == L.LLA_EINVAL      # fits with 4 channels, not with 8
    big = make_tables(8, wmax + 1, seed=2)
    db = dev_tables(big)
    s8 = in_table_symbols(big, 4, 1)
    assert device_encode(s8, db, wmax + 1, window=0)[0] == L.LLA_EINVAL
    assert device_decode_wide(pay, off, 0, 4, db, 8, wmax + 1, 0)[0] == L.LLA_EINVAL
    assert device_gather_wide(pay, off, 0, 4, np.arange(4), db, 8, wmax + 1, 0)[0] == L.LLA_EINVAL
    # null pointers
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = L.ptr(t)
    stride = int(lib.lla_rans_max_encoded_bytes(4))
    assert lib.lla_quantise_encode_wide(None, 0, 1, 4, None, None, None, p, 4, p, p, p, stride, p, None, 0, None) == L.LLA_EINVAL
    assert lib.lla_quantise_encode_wide(p, 2, 1, 4, None, p, p, p, 4, p, p, p, stride, p, None, 0, None) == L.LLA_EINVAL
    assert lib.lla_quantise_encode_wide(p, 0, 1, 4, None, None, None, None, 4, p, p, p, stride, p, None, 0, None) == L.LLA_EINVAL
    assert lib.lla_rans_decode_batch_wide(None, p, 0, 0, 1, 1, 4, p, 4, p, p, p, p, 0, None) == L.LLA_EINVAL
    assert lib.lla_rans_decode_batch_wide(p, p, 0, 0, 1, 1, 4, p, 4, p, p, None, p, 0, None) == L.LLA_EINVAL
    assert lib.lla_rans_decode_gather_wide(p, p, 0, 0, 1, 1, None, 1, 4, p, 4, p, p, p, p, p, p, 2, 4, p, 0, None) == L.LLA_EINVAL
    assert lib.lla_rans_decode_gather_wide(p, p, 0, 0, 1, 1, p, 1, 4, p, 4, p, p, p, p, p, p, 2, 4, None, 0, None) == L.LLA_EINVAL
    assert lib.lla_rans_decode_gather_wide(p, p, 0, 0, 1, 1, p, 1, 4, p, 4, p, p, p, p, p, p, 2, 3, p, 0, None) == L.LLA_EINVAL   # ld < C
    # B == 0: nothing to do
    assert lib.lla_quantise_encode_wide(p, 0, 0, 4, None, None, None, p, 4, p, p, p, stride, p, None, 0, None) == L.LLA_OK
    assert lib.lla_rans_decode_batch_wide(p, p, 0, 0, 1, 0, 4, p, 4, p, p, p, p, 0, None) == L.LLA_OK
    assert lib.lla_rans_decode_gather_wide(p, p, 0, 0, 1, 1, p, 0, 4, p, 4, p, p, p, p, p, p, 2, 4, p, 0, None) == L.LLA_OK


def test_oracle_agrees_on_a_small_case():
    """One record of the smallest shape against the pure-Python coder (oracle.pyrans), which shares no code with the library."""
    from oracle import pyrans
    C, W = SMALL
    tab, d, z, sym, pay, off, _ = small_reference(70, False)
    rc, s, ln, _ = device_encode(z[:3], d, W, window=8)
    assert rc == 0
    want = b"".join(pyrans.encode(sym[i], tab["cdf"], tab["cdf_len"], tab["offset"]) for i in range(3))
    assert s.tobytes() == want
    assert list(pyrans.decode(s.tobytes()[:int(ln[0])], C, tab["cdf"], tab["cdf_len"], tab["offset"])) == sym[0].tolist()

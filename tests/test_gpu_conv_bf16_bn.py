"""zsg_conv_igemm_bf16_bn / _bn_supported / zsg_conv_igemm_bf16_partial_rows (csrc/igemm_bf16.hip) through the C ABI: the bf16 MFMA
convolution with the fused BatchNorm partial rows [m_tiles][2][N] (enc_dtype = "bf16_fwd").

Bounds, none taken from what the code gives:
  * integer data (src in [-2, 2], weights in [-1, 1]), chosen so that every output and every tile's sum of squares stays below 2^24
    (make_case asserts both on the int64 reference, for BM = 64 and 128): every fp32 sum of such integers is exact in any order, so
    out and both partial rows must equal int64 arithmetic with zero tolerance;
  * standard-normal data: out must be bit-equal to zsg_conv_igemm_bf16's; a partial is compared with the fp64 column sum of the kernel's
    OWN out rows of that tile.  A tile sums at most BM values per column with BM - 1 fp32 additions (rows ascending inside a thread,
    row groups in index order: include/zsg.h), each off by at most 2^-24 of a partial sum that is at most sum |v|:
    |partial - ref| <= (BM - 1) * 2^-24 * sum |v|, and likewise (BM - 1) * 2^-24 * sum v^2 for the squares.
The tile -> partial-row attribution is computed here from zsg_conv_igemm_bf16_partial_rows and BM (one segment: tile t holds the rows
[t * BM, min(rows, (t + 1) * BM))).  Every case runs on the tile hints 0, 64x64, 128x64, 128x128."""
import ctypes as C
import functools
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

HINTS = (0, (64, 64), (128, 64), (128, 128))
SENTINEL = -12345.5
PAD_ROWS = 3            # sentinel rows kept behind the partial rows the launch may write

# name -> (H, W, B, C, N, k, stride, pad)
CASES = {
    "pw_tail": (9, 9, 2, 64, 256, 1, 1, 0),       # 162 rows: the last M tile partly invalid at BM 64 and 128
    "c3": (10, 10, 2, 64, 64, 3, 1, 1),           # 200 rows, N < BN at BN = 128; border taps
    "c3s2": (9, 9, 3, 128, 128, 3, 2, 1),         # 9x9 -> 5x5, 75 rows: a single partial tile at BM = 128
    "ds": (10, 10, 2, 64, 192, 1, 2, 0),          # 10x10 -> 5x5; a column tile past N (192 against 128 / 256)
    "full": (8, 8, 4, 256, 64, 1, 1, 0),          # 256 rows: exact multiples, several full tiles
}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, ops
    return _lib, ops


def conv_out(n, k, s, p):
    return (n + 2 * p - (k - 1) - 1) // s + 1


def conv_ref(src, w, k, s, p, Ho, Wo):
    """src [B, H, W, C], w [N, k, k, C] of one dtype (int64 / float64) -> [B, Ho, Wo, N], tap by tap in that dtype's own arithmetic"""
    B, H, W, Cc = src.shape
    buf = torch.zeros(B, H + 2 * p, W + 2 * p, Cc, dtype=src.dtype)
    buf[:, p:p + H, p:p + W] = src
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=src.dtype)
    for ty in range(k):
        for tx in range(k):
            win = buf[:, ty: ty + (Ho - 1) * s + 1: s, tx: tx + (Wo - 1) * s + 1: s]
            out += torch.matmul(win.reshape(-1, Cc), w[:, ty, tx].t()).view(B, Ho, Wo, -1)
    return out


@functools.lru_cache(maxsize=None)
def make_case(name, kind):
    """operands (fp32, CPU) of one case and, for integer data, the int64 reference — computed once, shared, never modified"""
    H, W, B, Cc, N, k, s, p = CASES[name]
    g = torch.Generator().manual_seed(300 + sorted(CASES).index(name) * 2 + (kind == "int"))
    Ho, Wo = conv_out(H, k, s, p), conv_out(W, k, s, p)
    # what the case is there for (the table above): its row count and how N sits against the 64- / 128-wide column tiles
    want_rows = {"pw_tail": 162, "c3": 200, "c3s2": 75, "ds": 50, "full": 256}[name]
    assert B * Ho * Wo == want_rows
    assert {"pw_tail": want_rows % 64 != 0 and want_rows % 128 != 0, "c3": N < 128, "c3s2": want_rows < 128,
            "ds": N % 128 != 0 and N % 64 == 0, "full": want_rows % 128 == 0}[name]
    if kind == "int":
        src = torch.randint(-2, 3, (B, H, W, Cc), generator=g).float()
        w = torch.randint(-1, 2, (N, k, k, Cc), generator=g).float()
        ref = conv_ref(src.to(torch.int64), w.to(torch.int64), k, s, p, Ho, Wo).view(-1, N)
        assert int(ref.abs().max()) < 2 ** 24
        for bm in (64, 128):          # every tile's sum of squares is exactly representable on the way
            sq = torch.stack([(ref[t:t + bm] ** 2).sum(0) for t in range(0, ref.shape[0], bm)])
            assert int(sq.max()) < 2 ** 24, f"{name}: tile sum of squares {int(sq.max())} >= 2^24"
    else:
        src = torch.randn(B, H, W, Cc, generator=g)
        w = torch.randn(N, k, k, Cc, generator=g)
        ref = None
    return dict(src=src, w=w, ref=ref, rows=B * Ho * Wo)


def pack(L, w):
    N, k, _, Cc = w.shape
    c8 = (Cc + 7) // 8 * 8
    wd = w.cuda()
    wp = torch.full((N, k * k, c8), 0x5555, dtype=torch.int16, device="cuda")
    job = struct.pack("<qqiiiiiiii", wd.data_ptr(), wp.data_ptr(), N, k * k, Cc, 0, Cc, c8, 0, 0)
    dev = torch.frombuffer(bytearray(job), dtype=torch.uint8).cuda()
    L.check(L.lib.zsg_pack_w_bf16_batched(dev.data_ptr(), 1, (N * k * k * c8 // 8 + 255) // 256, L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    return wp


def launch(Z, name, kind, hint, entry="bn"):
    """run one case; returns (out [rows, N], partial buffer [prow + PAD_ROWS, 2, N] or None, partial rows, BM)"""
    L, ops = Z
    H, W, B, Cc, N, k, s, p = CASES[name]
    cs = make_case(name, kind)
    Ho, Wo = conv_out(H, k, s, p), conv_out(W, k, s, p)
    src = cs["src"].reshape(-1).cuda()
    wp = pack(L, cs["w"])
    out = torch.full((B * Ho * Wo * N,), float("nan"), device="cuda")
    desc = ops.fwd_desc(ops.TView(src, B, Cc, Cc, [ops.Level(0, H, W, H * W * Cc)]), ops.TView(out, B, N, N, [ops.Level(0, Ho, Wo, Ho * Wo * N)]),
                        Cc, N, k, s, p, 1, wC=Cc, tile_hint=0 if hint == 0 else ops.tile_hint(hint[0], hint[1], 1))
    if entry == "plain":
        L.check(L.lib.zsg_conv_igemm_bf16(C.byref(desc), src.data_ptr(), wp.data_ptr(), out.data_ptr(), None, None, L.stream_ptr()), "bf16")
        torch.cuda.synchronize()
        return out.cpu().view(-1, N), None, 0, 0
    assert L.lib.zsg_conv_igemm_bf16_bn_supported(C.byref(desc)) == 1
    prow = int(L.lib.zsg_conv_igemm_bf16_partial_rows(C.byref(desc)))
    rows = cs["rows"]
    bms = [bm for bm in (64, 128) if (rows + bm - 1) // bm == prow]
    if hint != 0:
        assert bms and hint[0] in bms, f"{name} hint {hint}: {prow} partial rows for {rows} rows"
        bm = hint[0]
    else:
        assert bms, f"{name}: the heuristic's {prow} partial rows fit neither BM"
        bm = bms[0]                  # (where both BM give the same count — one tile — the attribution is the same too)
    part = torch.full((prow + PAD_ROWS, 2, N), SENTINEL, device="cuda")
    L.check(L.lib.zsg_conv_igemm_bf16_bn(C.byref(desc), src.data_ptr(), wp.data_ptr(), out.data_ptr(), part.data_ptr(), L.stream_ptr()), "bf16_bn")
    torch.cuda.synchronize()
    return out.cpu().view(-1, N), part.cpu(), prow, bm


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_is_exact(Z, name):
    cs = make_case(name, "int")
    ref = cs["ref"]
    for hint in HINTS:
        out, part, prow, bm = launch(Z, name, "int", hint)
        assert torch.equal(out.view(torch.int32), ref.float().view(torch.int32)), f"{name} hint {hint}: out"
        for t in range(prow):
            r = ref[t * bm:(t + 1) * bm]
            assert torch.equal(part[t, 0].double(), r.sum(0).double()), f"{name} hint {hint} tile {t}: sum"
            assert torch.equal(part[t, 1].double(), (r * r).sum(0).double()), f"{name} hint {hint} tile {t}: sum of squares"


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_data_out_bit_equal_and_partials_within_the_summation_bound(Z, name):
    worst = 0.0
    for hint in HINTS:
        out, part, prow, bm = launch(Z, name, "rand", hint)
        plain, _, _, _ = launch(Z, name, "rand", hint, entry="plain")
        assert not torch.isnan(out).any(), f"{name} hint {hint}: unwritten output elements"
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), f"{name} hint {hint}: out differs from zsg_conv_igemm_bf16"
        v = out.double()
        for t in range(prow):
            r = v[t * bm:(t + 1) * bm]
            for which, (ref, mag) in enumerate(((r.sum(0), r.abs().sum(0)), ((r * r).sum(0), (r * r).sum(0)))):
                err = (part[t, which].double() - ref).abs()
                bound = (bm - 1) * 2.0 ** -24 * mag
                frac = float((err / bound.clamp(min=1e-300)).max())
                worst = max(worst, frac)
                assert bool((err <= bound).all()), f"{name} hint {hint} tile {t} [{which}]: max error / bound = {frac:.3f}"
    print(f"bf16_bn {name}: largest |partial - fp64 sum| / bound over all tile hints = {worst:.4f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_nothing_written_outside_the_partial_rows(Z, name):
    N = CASES[name][4]
    for hint in HINTS:
        _, part, prow, _ = launch(Z, name, "rand", hint)
        assert part.shape == (prow + PAD_ROWS, 2, N)
        assert bool((part[prow:] == SENTINEL).all()), f"{name} hint {hint}: rows >= partial_rows changed"
        assert not bool((part[:prow] == SENTINEL).any()), f"{name} hint {hint}: an element of [m_tiles][2][N] was not written"


def test_two_runs_write_identical_bits(Z):
    for name in ("pw_tail", "c3"):
        for hint in HINTS:
            a, pa, _, _ = launch(Z, name, "rand", hint)
            b, pb, _, _ = launch(Z, name, "rand", hint)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(pa.view(torch.int32), pb.view(torch.int32)), (name, hint)


def test_refusals_launch_nothing(Z):
    L, ops = Z
    x = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    o = torch.full((2 * 8 * 8 * 64,), 3.0, device="cuda")
    part = torch.full((8 * 2 * 64 + 4,), SENTINEL, device="cuda")
    wp = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    lv = [ops.Level(0, 8, 8, 8 * 8 * 64)]

    def desc(N=64, **kw):
        d = ops.fwd_desc(ops.TView(x, 2, 64, 64, lv), ops.TView(o, 2, N, 64, lv), 64, N, 1, 1, 0, 1, wC=64)
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d
    bad = {
        "relu": desc(relu=1),
        "N % 4": desc(N=62),
        "merge_x": desc(merge_x=1),
        "split-K": desc(tile_hint=ops.tile_hint(64, 64, 2)),
        "epi_flags": desc(epi_flags=1),
        "out_ld % 4": desc(out_ld=66),
    }
    for what, d in bad.items():
        assert L.lib.zsg_conv_igemm_bf16_bn_supported(C.byref(d)) == 0, what
        assert L.lib.zsg_conv_igemm_bf16_partial_rows(C.byref(d)) == -1, what
        rc = L.lib.zsg_conv_igemm_bf16_bn(C.byref(d), x.data_ptr(), wp.data_ptr(), o.data_ptr(), part.data_ptr(), L.stream_ptr())
        msg = L.lib.zsg_last_error().decode()
        assert rc == -1 and "conv_igemm_bf16_bn" in msg and len(msg) > 30, (what, rc, msg)
    good = desc()
    assert L.lib.zsg_conv_igemm_bf16_bn_supported(C.byref(good)) == 1
    assert L.lib.zsg_conv_igemm_bf16_partial_rows(C.byref(good)) in (1, 2)          # 128 rows: one or two tiles
    for what, (op, pp) in {"misaligned partials": (o.data_ptr(), part.data_ptr() + 4), "null partials": (o.data_ptr(), None),
                           "misaligned out": (o.data_ptr() + 4, part.data_ptr())}.items():
        rc = L.lib.zsg_conv_igemm_bf16_bn(C.byref(good), x.data_ptr(), wp.data_ptr(), op, pp, L.stream_ptr())
        msg = L.lib.zsg_last_error().decode()
        assert rc == -1 and "conv_igemm_bf16_bn" in msg and ("bn_partials" in msg or "out" in msg), (what, rc, msg)
    torch.cuda.synchronize()
    assert float(o.min()) == 3.0 and float(o.max()) == 3.0, "a refused call must launch nothing"
    assert bool((part == SENTINEL).all()), "a refused call must launch nothing"
    good.tile_hint = ops.tile_hint(64, 64, 1)
    assert L.lib.zsg_conv_igemm_bf16_partial_rows(C.byref(good)) == 2
    assert L.lib.zsg_conv_igemm_bf16_bn(C.byref(good), x.data_ptr(), wp.data_ptr(), o.data_ptr(), part.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0 and float(part[:2 * 2 * 64].abs().max()) == 0.0 and bool((part[2 * 2 * 64:] == SENTINEL).all())

"""Exact-arithmetic, guarded tests of the fp32 convolution kernels through the C ABI: zsg_conv_igemm (implicit-GEMM tiles, atomic
split-K, stream-K, the filter-resident streaming kernels behind BM = 32), zsg_conv_wino + zsg_wino_weights, zsg_conv_wgrad,
zsg_conv_wgrad_wino / _batched, zsg_transpose_w / _batched.

Data are small non-zero integers (tests/conv_exact_ref.py): every product and every partial sum is exact in fp32 — fp32 MFMA, atomic
split-K, stream-K fix-up, slab reduction and the Winograd transforms (constants +-1, +-1/2) included — so EVERY variant of EVERY entry
must equal the integer reference bit for bit, and therefore every other variant; two runs of one launch write identical bits, atomic
split-K included (a property of the integer data, not of the atomics).  tests/test_cpu_conv_exact.py proves the bounds that make this
so from the reference alone.  Every comparison here is an equality; there is no tolerance in this file.

Every operand sits between NaN guards with finite poison (2^20) on everything the descriptor does not address, every output between
sentinels with NaN where the launch must write: a read past a ragged tile, a K tail or a level boundary, or a stray store, destroys
the equality.  expected_rc() — written from include/zsg.h and the entries' requirement messages — says for every (case, variant,
epilogue) whether the library must run it (0) or refuse it (-1); the library's return code must agree, a refused launch must leave
every output byte untouched and set zsg_last_error.  Nothing is skipped silently.

Not covered: an out-of-range read whose value never reaches a result is not detected by guards; rounding on non-integer data stays
with the Gaussian-data tests (test_gpu_ops.py, test_gpu_wino.py, test_gpu_streamk.py); the BatchNorm-fused siblings (_bnb, _bnpre,
_bnstat, _tail) are held to the same method by tests/test_gpu_conv_bn_exact.py.

Split-K and the accumulate + mask epilogue (include/zsg.h): every K slice adds its own masked term to what `out` holds, so the launch
computes prev + mask * sum, which is the documented (prev + sum) * mask exactly when prev is zero wherever mask <= 0 — what the
training plans hold in dx, every earlier writer having applied the same mask.  The split-K variants are tested with such a prev
(epilogue `acc_mask_z`), the unsplit ones with an arbitrary one."""
import ctypes as C
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_exact_ref as R  # noqa: E402
from test_gpu_ops import WS, Z, stream_scratch  # noqa: E402,F401

NAMES = [c.name for c in R.CASES]
NUM_CU = 256
_STATE = {}


@pytest.fixture
def X(Z):
    """the library on a stream of this module's own whose stream-K scratch holds the largest launch (768 slots of 128x128)"""
    L, ops = Z
    if "stream" not in _STATE:
        _STATE["stream"] = torch.cuda.Stream()
        stream_scratch(L, _STATE["stream"].cuda_stream, mb=64)
    with torch.cuda.stream(_STATE["stream"]):
        yield L, ops
    torch.cuda.synchronize()


# ---- device operands ------------------------------------------------------------------------------------------------------------------
class Dev:
    """a conv_exact_ref.Buf on the device; ptr = its first operand element"""

    def __init__(self, buf, t=None):
        self.buf = buf
        self.t = buf.t.cuda() if t is None else t

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.buf.lo

    def clone(self):
        return Dev(self.buf, self.t.clone())


def inp(extent, idx, data):
    return Dev(R.build_input(extent, idx, data[idx]))


def cdesc(L, D, hint=0, relu=0):
    d = L.ConvDesc()
    d.B, d.C, d.N, d.src_ld, d.out_ld = D.B, D.C, D.N, D.src_ld, D.out_ld
    d.wR, d.wS, d.wC, d.wc0, d.wt_ld = D.wR, D.wS, D.wC, D.wc0, D.wt_ld
    d.relu, d.merge_x, d.nseg, d.tile_hint = int(relu), D.merge_x, D.nseg, hint
    for i, g in enumerate(D.segs):
        s = d.seg[i]
        for f in ("rows_y", "rows_x", "src_H", "src_W", "sy", "sx", "out_W", "osy", "osx", "opy", "opx", "src_off", "src_bstride",
                  "out_off", "out_bstride"):
            setattr(s, f, getattr(g, f))
        s.ty = L.Taps(g.ty.n, g.ty.w0, g.ty.wstep, g.ty.d0, g.ty.dstep)
        s.tx = L.Taps(g.tx.n, g.tx.w0, g.tx.wstep, g.tx.d0, g.tx.dstep)
    return d


def explain(what, got, exp, lo, D=None):
    """first differing element: flat index, and (output of a convolution) its segment, image, pixel, channel and 64-row tile; the K
    position of a wrong sum cannot be read off the output"""
    g, e = got.cpu(), exp.cpu()
    bad = ((g != e) | torch.isnan(g)).nonzero().view(-1)
    i = int(bad[0])
    msg = f"{what}: {len(bad)} of {g.numel()} elements differ; first at buffer index {i} (operand element {i - lo}): got {float(g[i])!r}, want {float(e[i])!r}"
    if i < lo or i >= g.numel() - R.GUARD:
        msg += " — inside a guard"
    elif float(e[i]) == R.SENTINEL:
        msg += " — a sentinel (an element the launch must not write)"
    if D is not None:
        for si in range(D.nseg):
            hit = (R.out_index(D, si) == i - lo).nonzero()
            if len(hit):
                b, y, x, n = map(int, hit[0])
                row = (b * D.segs[si].rows_y + y) * D.segs[si].rows_x + x
                msg += f" — segment {si} image {b} row (y {y}, x {x}) channel {n}: GEMM row {row} (64-row tile {row // 64}), column tile {n // 64}"
    return msg


def same(what, got: Dev, exp, D=None):
    if not torch.equal(got.t, exp):
        raise AssertionError(explain(what, got.t, exp, got.buf.lo, D))


def untouched(what, got: Dev, before):
    """a refused launch: every byte as it was (NaN pre-fill included, hence the comparison of the bit patterns)"""
    if not torch.equal(got.t.view(torch.int32), before.view(torch.int32)):
        g, b = got.t.view(torch.int32).cpu(), before.view(torch.int32).cpu()
        i = int((g != b).nonzero()[0])
        raise AssertionError(f"{what}: buffer index {i} (operand element {i - got.buf.lo}) changed to {float(got.t[i])!r}")


class Tally:
    def __init__(self):
        self.ran = self.refused = 0

    def report(self, what):
        print(f"{what}: {self.ran} (variant, epilogue) launches compared at zero tolerance, {self.refused} refused as expected")


# ---- tile variants --------------------------------------------------------------------------------------------------------------------
def ig_hint(v):
    if v is None:
        return 0
    bm, bn, w8, k64, sp, sk = v
    return bm | (bn << 8) | (sp << 16) | (w8 << 24) | (k64 << 27) | (sk << 28)


TILES = [(64, 64), (128, 64), (128, 128)]
SK_FORMS = [(64, 64, 0, 0), (64, 64, 1, 0), (64, 64, 1, 1), (128, 64, 1, 0), (128, 128, 1, 0), (128, 128, 0, 0)]      # conv_igemm_impl
IG_VARIANTS = ([None]
               + [(bm, bn, w8, k64, 1, 0) for bm, bn in TILES for w8 in (0, 1) for k64 in (0, 1)]
               + [(bm, bn, 0, 0, sp, 0) for bm, bn in TILES for sp in (2, 3, 5, 8)]            # atomic split-K on every tile
               + [(64, 64, 1, 1, 2, 0), (64, 64, 1, 1, 5, 0), (128, 64, 1, 0, 3, 0), (128, 128, 1, 1, 2, 0)]
               + [f + (1, sk) for f in SK_FORMS for sk in (1, 2, 3)]
               + [(32, 32, 0, 0, 1, 0), (32, 64, 0, 0, 1, 0), (32, 128, 0, 0, 1, 0)])         # the streaming kernels (pw unit widths; mx)
IG_REFUSED = [(128, 64, 0, 0, 1, 1), (64, 64, 0, 1, 1, 2), (96, 64, 0, 0, 1, 0), (64, 128, 0, 0, 1, 0), (64, 128, 1, 0, 1, 0),
              (32, 64, 0, 0, 2, 0), (64, 64, 0, 0, 2, 1), (32, 64, 0, 0, 1, 1),
              # a tile that does not exist TOGETHER with split-K: refused before the split-K preparation zeroes the output
              (96, 64, 0, 0, 2, 0), (64, 128, 1, 0, 3, 0), (64, 128, 0, 0, 5, 0)]
EPIS = ["plain", "bias_relu", "add", "add_alias", "mask", "stats"]


def pw_ok(D, uw):
    """csrc/pw.hip's geometry (include/zsg.h: 'the 1x1 / stride-1 convolutions whose filter fits a CU's LDS'): one dense 1x1 / stride-1
    segment, C % 64 == 0, N a multiple of the unit width, the filter cut into 1, 2, 4 or 8 panels of 1, 2, 4 or 8 units that fit
    160 KB next to the eight 32 x 68 wave buffers, 16-byte aligned rows"""
    if D.nseg != 1 or D.merge_x:
        return False
    g = D.segs[0]
    if (g.ty.n, g.tx.n, g.ty.d0, g.tx.d0, g.sy, g.sx, g.osy, g.osx, g.opy, g.opx) != (1, 1, 0, 0, 1, 1, 1, 1, 0, 0):
        return False
    if g.src_H != g.rows_y or g.src_W != g.rows_x or g.out_W != g.rows_x or g.src_bstride != g.rows_y * g.rows_x * D.src_ld \
            or g.out_bstride != g.rows_y * g.rows_x * D.out_ld:
        return False
    if uw not in (32, 64, 128) or D.C % 64 or D.N % uw:
        return False
    ncb = 0
    c = 1
    while c <= 8 and not ncb:
        if D.N % c or (D.N // c) % uw:
            break
        nb = D.N // c
        if nb // uw in (1, 2, 4, 8) and (nb * (D.C + 4) + 8 * 32 * 68) * 4 <= 160 * 1024:
            ncb = c
        c *= 2
    if not ncb:
        return False
    return not (D.src_ld % 4 or D.out_ld % 4 or g.src_off % 4 or g.out_off % 4 or D.wt_ld % 4 or D.wc0 % 4)


def mx_ok(D):
    """csrc/mx.hip's geometry: one merge_x segment (C = src_ld = wC = 4), a 7x7 / 7x8 or 3x(1..4) window of unit-step x taps, 64 output
    channels in dense, 16-byte aligned pixel rows"""
    if not D.merge_x or D.nseg != 1:
        return False
    g = D.segs[0]
    if D.C != 4 or D.src_ld != 4 or D.wC != 4 or D.wc0 or not 1 <= g.tx.n <= 8 or g.tx.dstep != 1 or g.tx.wstep != 1 or g.tx.w0 or D.wS != g.tx.n:
        return False
    if not ((g.ty.n == 7 and g.tx.n >= 7) or (g.ty.n == 3 and g.tx.n <= 4)) or g.ty.w0 or g.ty.wstep != 1 or g.ty.dstep < 1:
        return False
    if D.N != 64 or (g.osy, g.osx, g.opy, g.opx) != (1, 1, 0, 0) or g.out_W != g.rows_x or g.out_bstride != g.rows_y * g.rows_x * D.out_ld:
        return False
    return not (D.out_ld % 4 or g.out_off % 4 or D.wt_ld % 4 or g.src_off % 4 or g.src_bstride % 4)


def vec_ok(D, unaligned):
    """16-byte addressable output rows: what the vectorised epilogue, stream-K and the Winograd statistics need"""
    return D.out_ld % 4 == 0 and D.N % 4 == 0 and not unaligned and all(g.out_off % 4 == 0 and g.out_bstride % 4 == 0 for g in D.segs)


def dense_out(D):
    g = D.segs[0]
    return D.nseg == 1 and D.out_ld == D.N and g.osy == 1 and g.osx == 1 and g.out_W == g.rows_x and g.out_bstride == g.rows_y * g.rows_x * D.N


def expected_rc(D, v, epi, unaligned=False):
    """0 / -1 of zsg_conv_igemm for descriptor D, tile variant v (None: hint 0) and epilogue epi, from include/zsg.h:
    split_k > 1: a single dense segment, no ReLU; stream-K: an implicit-GEMM tile of the six instantiated forms, one segment, no
    split-K, 16-byte addressable output rows, fewer tiles than 256 x workgroups-per-CU; BM = 32: the streaming kernels' geometries,
    16-byte aligned operands, no split-K, (merge_x) no add / mask operand; bn_partials: a plain, unsplit convolution; tiles other than
    64x64 / 128x64 / 128x128 do not exist (merge_x: BM = 128 runs the 128x64 tile and every other BM the 64x64 one, the 8-wave and
    64-deep-K bits are ignored)."""
    relu = bias = epi == "bias_relu"
    add = epi in ("add", "add_alias", "acc_mask", "acc_mask_z")
    mask = epi in ("mask", "acc_mask", "acc_mask_z")
    stats = epi == "stats"
    if v is None:
        return 0
    bm, bn, w8, k64, sp, sk = v
    if sk and (bm == 32 or D.merge_x or D.nseg != 1 or sp > 1):
        return -1
    if bm == 32:
        if sp > 1:
            return -1
        if D.merge_x:
            ok = mx_ok(D) and not add and not mask
        else:
            ok = pw_ok(D, bn)
        return 0 if ok and not unaligned and not (stats and (bias or add or relu or mask)) else -1
    if D.merge_x:
        bn, w8, k64 = min(bn, 64), 0, 0
    if stats and (sp > 1 or bias or add or relu):
        return -1
    if sp > 1 and (relu or not dense_out(D)):
        return -1
    if sk:
        rows = D.B * D.segs[0].rows_y * D.segs[0].rows_x
        if not vec_ok(D, unaligned) or -(-rows // bm) * -(-D.N // bn) > NUM_CU * sk or (bm, bn, w8, k64) not in SK_FORMS:
            return -1
        return 0
    if D.merge_x:
        return 0          # (BM = 128 runs the 128x64 tile, every other BM the 64x64 one)
    return 0 if (bm, bn) in TILES else -1


WN_VARIANTS = ([None] + [(tb, bn, ps4, 1, 0) for tb in (32, 64) for bn in (32, 64) for ps4 in (0, 1)]
               + [(64, 64, 0, 2, 0), (32, 64, 1, 3, 0), (32, 32, 0, 2, 0), (64, 32, 1, 5, 0)] + [(32, 64, 1, 1, 1)])
WN_REFUSED = [(64, 64, 1, 1, 1), (32, 64, 0, 1, 1), (128, 64, 0, 1, 0),
              (32, 64, 1, 2, 1), (64, 64, 0, 3, 1)]          # stream-K together with split-K: refused before the output is zeroed


def wn_hint(v):
    if v is None:
        return 0
    tb, bn, ps4, sp, sk = v
    return tb | (bn << 8) | (sp << 16) | (ps4 << 24) | (sk << 28)


def expected_rc_wino(D, v, epi, unaligned=False):
    """zsg_conv_wino: tiles {32, 64}^2; bn_partials: plain, unsplit, 16-byte addressable rows; split-K: a single dense segment, no ReLU;
    stream-K: the 32 x 64 four-group tile only, one segment, no split-K, 16-byte addressable rows, at most 256 tiles"""
    relu = bias = epi == "bias_relu"
    add = epi in ("add", "add_alias", "acc_mask", "acc_mask_z")
    stats = epi == "stats"
    tb, bn, ps4, sp, sk = v or (64, 64, 0, 1, 0)
    if tb not in (32, 64) or bn not in (32, 64):
        return -1
    if stats and (sp > 1 or bias or add or relu or not vec_ok(D, unaligned)):
        return -1
    g = D.segs[0]
    if sp > 1 and (relu or D.nseg != 1 or D.out_ld != D.N or g.out_bstride != g.rows_y * g.rows_x * D.N):
        return -1
    if sk:
        tiles = sum(-(-D.B * ((s.src_H + 1) // 2) * ((s.src_W + 1) // 2) // tb) for s in D.segs) * -(-D.N // bn)
        if sp > 1 or not vec_ok(D, unaligned) or D.nseg != 1 or (tb, bn, ps4) != (32, 64, 1) or tiles > NUM_CU:
            return -1
    return 0


# ---- one launch of a forward-type entry (zsg_conv_igemm / zsg_conv_wino), all epilogues ------------------------------------------------
class FwdSide:
    """the operands of one descriptor D (a forward, or a data gradient seen as the forward it is) on the device, and per epilogue the
    initial output buffer and the complete expected buffer"""

    def __init__(self, D, src, wt, bias, add, mask, rows, shift=0):
        self.D, self.rows, self.shift = D, rows, shift
        self.src = Dev(R.build_input(R.src_extent(D), R.src_addressed(D), src[R.src_addressed(D)]))
        self.wt_host = wt
        self.wt = Dev(R.build_input(R.wt_extent(D), R.wt_index(D), wt[R.wt_index(D)]))
        self.written = R.out_written(D)
        ext = R.out_extent(D)
        self.bias_h, self.add_h, self.mask_h = bias, add, mask
        self.bias = Dev(R.build_input(D.N, torch.arange(D.N), bias))
        self.add = Dev(R.build_input(ext, self.written, add[self.written]))
        self.mask = Dev(R.build_input(ext, self.written, mask[self.written]))
        self.src_h = src
        self._epi = {}

    def epi(self, name):
        """(init Dev, expected full buffer on the device, relu, bias ptr, add Dev or 'out' or None, mask Dev or None)"""
        if name not in self._epi:
            D, w = self.D, self.written
            relu = name == "bias_relu"
            bias = self.bias_h if name == "bias_relu" else None
            add = self.add_h if name in ("add", "add_alias", "acc_mask", "acc_mask_z") else None
            mask = self.mask_h if name in ("mask", "acc_mask", "acc_mask_z") else None
            alias = name in ("add_alias", "acc_mask", "acc_mask_z")
            if name == "acc_mask_z":          # prev is zero wherever mask <= 0 (see the module docstring)
                add = torch.where(mask > 0, add, torch.zeros_like(add))
            init = R.build_output(R.out_extent(D), w, add[w] if alias else None, self.shift)
            ref = torch.zeros(R.out_extent(D), dtype=R.DT)
            for si, acc in enumerate(self.rows):
                oi = R.out_index(D, si)
                ref[oi] = R.epilogue(acc, bias, None if add is None else add[oi], relu, None if mask is None else mask[oi])
            exp = R.expected_output(init, ref, w).cuda()
            self._epi[name] = (Dev(init), exp, relu, self.bias.ptr if bias is not None else None,
                               None if add is None else ("out" if alias else self.add), self.mask if mask is not None else None)
        return self._epi[name]


def stale_error(L):
    """leaves a known message of ANOTHER entry in zsg_last_error, so that a refusal's own message can be told from a left-over"""
    assert L.lib.zsg_wino_weights(None, 0, 0, None) != 0
    return L.lib.zsg_last_error()


def refusal_message(L, stale, what):
    msg = L.lib.zsg_last_error()
    assert msg and msg != stale, f"{what}: a refused launch must set zsg_last_error itself (it reads {msg!r})"
    return msg.decode()


def part_buf(rows, N):
    return Dev(R.build_output(rows * 2 * N, torch.arange(rows * 2 * N)))


def run_fwd_entry(L, fn, side: FwdSide, wt_ptr, hint, epi, want_rc, tally, what, part_ref=None, part_rows=None, totals_only=False):
    """one (variant, epilogue): the launch, its return code against the prediction, the complete output buffer against the expected one
    (or, refused: against what was there before), bn_partials likewise, and the same launch once more for identical bits"""
    init, exp, relu, bias, add, mask = side.epi("plain" if epi == "stats" else epi)
    d = cdesc(L, side.D, hint, relu)
    st = L.stream_ptr()
    part = None
    if epi == "stats":
        prow = part_rows if part_rows and part_rows > 0 else 1
        part = part_buf(prow, side.D.N)
        part0 = part.t.clone()
    outs = []
    for rep in range(2):
        out = init.clone()
        if part is not None and rep:
            part = Dev(part.buf, part0.clone())
        stale = stale_error(L) if want_rc else None
        rc = fn(C.byref(d), side.src.ptr, wt_ptr, out.ptr, bias, out.ptr if add == "out" else (add.ptr if add else None),
                mask.ptr if mask else None, part.ptr if part is not None else None, st)
        assert rc == want_rc, f"{what}: return code {rc}, expected {want_rc} ({L.lib.zsg_last_error().decode()})"
        if rc != 0:
            assert "conv" in refusal_message(L, stale, what)
            untouched(f"{what}: refused, yet the output changed", out, init.t)
            if part is not None:
                untouched(f"{what}: refused, yet bn_partials changed", part, part0)
            tally.refused += 1
            return
        same(what, out, exp, side.D)
        if part is not None:
            if totals_only:       # pw / mx: one partial row per workgroup — the column totals are the contract, and the row count
                got = part.t[part.buf.lo:part.buf.lo + part.buf.extent].view(prow, 2, side.D.N)
                assert not torch.isnan(got).any(), f"{what}: NaN in a written partial row"
                assert torch.equal(got.sum(0).cpu().double(), part_ref.sum(0)), f"{what}: bn_partials column totals"
                same(f"{what}: bn_partials guards", Dev(part.buf, torch.cat([part.t[:part.buf.lo], part.t[part.buf.lo + part.buf.extent:]])),
                     torch.full((2 * R.GUARD,), R.SENTINEL, device="cuda"))
            else:
                same(f"{what}: bn_partials", part, R.expected_output(part.buf, part_ref.reshape(-1), torch.arange(part.buf.extent)).cuda())
        outs.append((out.t, None if part is None else part.t))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), f"{what}: two runs differ"
    if part is not None:
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), f"{what}: two runs' bn_partials differ"
    tally.ran += 1


def igemm_all(L, ops, side: FwdSide, variants, epis, tally, what, unaligned=False):
    ran = set()
    for v in variants:
        for epi in epis:
            if v is not None and v[4] > 1 and epi == "acc_mask":
                epi = "acc_mask_z"          # (split-K: prev + mask * sum, the documented epilogue for a prev that is zero where mask <= 0)
            if v is None and epi == "stats":
                continue          # (no hint, no promise about the partial rows: zsg_conv_igemm_partial_rows returns -1)
            if side.D.merge_x and v is not None and v[0] != 32 and (v[0], v[1]) not in TILES:
                continue          # (merge_x maps ANY tile field onto its 64x64 / 128x64 kernels, include/zsg.h: not a refusal, and no tile of its own)
            want = expected_rc(side.D, v, epi, unaligned)
            pref = prow = None
            totals = False
            if epi == "stats":
                d = cdesc(L, side.D, ig_hint(v))
                prow = int(L.lib.zsg_conv_igemm_partial_rows(C.byref(d)))
                if v[0] == 32:
                    totals = True
                    if want == 0:
                        assert prow > 0, f"{what} {v}: zsg_conv_igemm_partial_rows must cover what the launch accepts"
                    pref = R.tile_partials(side.rows, 1 << 30)
                    pref = pref.sum(0, keepdim=True)
                else:
                    pref = R.tile_partials(side.rows, v[0])
                    assert prow == pref.shape[0], f"{what} {v}: zsg_conv_igemm_partial_rows {prow}, the layout has {pref.shape[0]}"
            before = tally.ran
            run_fwd_entry(L, L.lib.zsg_conv_igemm, side, side.wt.ptr, ig_hint(v), epi, want, tally, f"{what} variant {v} {epi}", pref, prow, totals)
            if tally.ran > before:
                ran.add(v)
    return ran


def fwd_side(cd, shift=0):
    return FwdSide(cd.F, cd.x, cd.w, cd.bias, cd.add, cd.mask, cd.fwd_rows(), shift)


def dg_side(cd):
    return FwdSide(cd.G, cd.dy_d, cd.wt.reshape(-1), torch.zeros(cd.G.N, dtype=R.DT), cd.prev, cd.dmask, cd.dg_rows())


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def test_descriptors_match_the_host_layer(X):
    """the descriptors the tests launch are, byte for byte, what ops.fwd_desc / ops.dgrad_desc build for the same views"""
    L, ops = X
    for c in R.CASES:
        tv = lambda v: ops.TView(torch.empty(1), v.B, v.C, v.ld, [ops.Level(l.off, l.H, l.W, l.bstride) for l in v.levels])
        a = ops.fwd_desc(tv(c.src_view()), tv(c.out_view()), c.C, c.N, c.k, c.s, c.p, c.d, wC=c.wC, wt_ld=c.wt_ld, wc0=c.wc0, merge_x=c.merge_x)
        assert bytes(a) == bytes(cdesc(L, c.fwd())), c.name
        if not c.merge_x:
            b = ops.dgrad_desc(tv(c.out_view(c.dy_ld)), tv(c.src_view()), c.dy_ld, c.C, c.k, c.s, c.p, c.d)
            g = c.dg()
            assert bytes(b) == bytes(cdesc(L, g)) and bool(b.zero_fill) == g.zero_fill, c.name


@pytest.mark.parametrize("name", NAMES)
def test_igemm_forward_exact(X, name):
    L, ops = X
    cd = R.case_data(name)
    c = cd.c
    t = Tally()
    side = fwd_side(cd, c.out_shift)
    epis = EPIS
    ran = igemm_all(L, ops, side, IG_VARIANTS + IG_REFUSED, epis, t, f"{name} forward", unaligned=c.out_shift != 0)
    assert None in ran, "every case runs the heuristic (hint 0)"
    # the tuner's streaming candidates are among the variants that ran
    for h in ops.pw_cands(cdesc(L, cd.F)):
        assert any(v is not None and ig_hint(v) == h for v in ran), hex(h)
    t.report(f"zsg_conv_igemm forward {name}")


@pytest.mark.parametrize("name", [n for n in NAMES if not R.CASE[n].merge_x])
def test_igemm_dgrad_exact(X, name):
    """the data gradient (stride-parity segments, zero_fill, C_red = dy.ld with operand zeros in the pad lanes), plain and with the
    accumulate + mask epilogue (add_src aliasing dx)"""
    L, ops = X
    cd = R.case_data(name)
    t = Tally()
    side = dg_side(cd)
    ran = igemm_all(L, ops, side, IG_VARIANTS + IG_REFUSED, ["plain", "acc_mask", "add_alias"], t, f"{name} dgrad")
    assert None in ran
    t.report(f"zsg_conv_igemm dgrad {name}")


def make_u(L, ops, src_ptr, N, Cred, row_ld, tap_ld, flip):
    """zsg_wino_weights into a NaN-filled, sentinel-guarded buffer; returns (Dev, the [chunks][16][Npad][8] view)"""
    n = int(L.lib.zsg_wino_u_elems(Cred, N))
    U = Dev(R.build_output(n, torch.arange(n)))
    jobs = ops.WinoJobs()
    jobs.add(src_ptr, U.ptr, N, Cred, row_ld, tap_ld, flip)
    jobs.finish("cuda")
    jobs.launch(L.stream_ptr())
    return U, jobs


def u_layout(img, N, Cred):
    """conv_exact_ref.wino_filter_image [n][4][4][c] in zsg_wino_weights' layout [ceil(C/8)][16][roundup(N,64)][8]: position 4*j + i holds
    element (i, j), negated for i = 3 (the kernel's input transform produces -V in that row), zeros beyond N and C"""
    chunks, npad = (Cred + 7) // 8, (N + 63) // 64 * 64
    u = torch.zeros(chunks, 16, npad, 8, dtype=R.DT)
    full = torch.zeros(npad, 4, 4, chunks * 8, dtype=R.DT)
    full[:N, :, :, :Cred] = img
    full[:, 3] = -full[:, 3]
    for i in range(4):
        for j in range(4):
            u[:, 4 * j + i] = full[:, i, j].view(npad, chunks, 8).permute(1, 0, 2)
    return u.reshape(-1)


def wino_all(L, ops, side, U, variants, epis, tally, what, unaligned=False):
    ran = set()
    for v in variants:
        for epi in epis:
            if v is not None and v[3] > 1 and epi == "acc_mask":
                epi = "acc_mask_z"
            want = expected_rc_wino(side.D, v, epi, unaligned)
            pref = prow = None
            if epi == "stats":
                tb = v[0] if v else 64
                if tb not in (32, 64):
                    continue
                pref = R.wino_tile_partials(side.rows, tb)
                prow = pref.shape[0]
            before = tally.ran
            run_fwd_entry(L, L.lib.zsg_conv_wino, side, U.ptr, wn_hint(v), epi, want, tally, f"{what} variant {v} {epi}", pref, prow)
            if tally.ran > before:
                ran.add(v)
    return ran


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASE[n].wino])
def test_wino_forward_dgrad_exact(X, name):
    """zsg_wino_weights (plain, and flipped from the transposed image) exactly, then zsg_conv_wino forward and data gradient on them"""
    L, ops = X
    cd = R.case_data(name)
    c = cd.c
    t = Tally()
    side = fwd_side(cd, c.out_shift)
    U, _ = make_u(L, ops, side.wt.ptr + 4 * c.wc0, c.N, c.C, c.wt_ld, c.wC, False)
    uref = u_layout(R.wino_filter_image(cd.w_dense), c.N, c.C)
    same(f"{name}: zsg_wino_weights", U, R.expected_output(U.buf, uref, torch.arange(U.buf.extent)).cuda())
    epis = EPIS
    ran = wino_all(L, ops, side, U, WN_VARIANTS + WN_REFUSED, epis, t, f"{name} wino forward", unaligned=c.out_shift != 0)
    assert None in ran
    ds = dg_side(cd)
    Ut, _ = make_u(L, ops, ds.wt.ptr, c.C, c.dy_ld, 9 * c.dy_ld, c.dy_ld, True)
    utref = u_layout(R.wino_filter_image(cd.wt, flip=True), c.C, c.dy_ld)
    same(f"{name}: zsg_wino_weights (flipped)", Ut, R.expected_output(Ut.buf, utref, torch.arange(Ut.buf.extent)).cuda())
    ran = wino_all(L, ops, ds, Ut, WN_VARIANTS + WN_REFUSED, ["plain", "acc_mask", "add_alias"], t, f"{name} wino dgrad")
    assert None in ran
    t.report(f"zsg_conv_wino forward + dgrad {name}")


WG_VARIANTS = ([0] + [(bm, bn, sp, 0, 0) for bm in (64, 128) for bn in (64, 128) for sp in (1, 2, 3, 16)]
               + [(128, 128, sp, w8, k32) for sp in (1, 3) for w8, k32 in ((1, 0), (0, 1), (1, 1))]
               + [(64, 255, 1, 0, 0), (64, 255, 2, 0, 0), (64, 255, 3, 0, 1)])


def wg_hint(v):
    return 0 if v == 0 else v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24) | (v[4] << 25)


class WgSide:
    """the weight gradient's operands for descriptor W (default: the case's, dy in dy_ld-wide rows; the same dy values in rows of
    another width give the same gradient) and, per accumulate flag, the initial dw buffer and the complete expected one"""

    def __init__(self, cd, W=None):
        W = W or cd.W
        self.W = W
        self.src = inp(R.src_extent(W), cd.x_idx, cd.x)
        g_idx = R.out_written(W)
        dy = torch.full((R.out_extent(W),), R.POISON, dtype=R.DT)
        dy[g_idx] = cd.dy_w[cd.g_idx]
        self.dy = inp(R.out_extent(W), g_idx, dy)
        ext = R.wt_extent(W)
        wi = cd.w_idx.reshape(-1)
        self.init, self.exp = {}, {}
        for acc in (0, 1):
            b = R.build_output(ext, wi, cd.dw_prev.reshape(-1) if acc else None)
            ref = torch.zeros(ext, dtype=R.DT)
            ref[cd.w_idx] = cd.dw() + (cd.dw_prev if acc else 0)
            self.init[acc], self.exp[acc] = Dev(b), R.expected_output(b, ref, wi).cuda()


def run_wgrad(L, fn, ws_: WgSide, hint, acc, tally, what, want_rc=0):
    d = cdesc(L, ws_.W, hint)
    outs = []
    for rep in range(2):
        dw = ws_.init[acc].clone()
        stale = stale_error(L) if want_rc else None
        rc = fn(C.byref(d), ws_.src.ptr, ws_.dy.ptr, dw.ptr, acc, WS.data_ptr(), WS.numel() * 4, L.stream_ptr())
        assert rc == want_rc, f"{what}: return code {rc}, expected {want_rc} ({L.lib.zsg_last_error().decode()})"
        if rc != 0:
            assert "conv_wgrad" in refusal_message(L, stale, what)
            untouched(f"{what}: refused, yet dw changed", dw, ws_.init[acc].t)
            tally.refused += 1
            return
        same(what, dw, ws_.exp[acc])          # (covers dw outside the channel window and the wt_ld slack: sentinels)
        outs.append(dw.t)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{what}: two runs differ"
    tally.ran += 1


@pytest.mark.parametrize("name", NAMES)
def test_wgrad_exact(X, name):
    """zsg_conv_wgrad: every tile, the 8-wave and 32-pixel-K forms, the 256-column tile, splits 1 / 2 / 3 / 16, accumulate on and off;
    the entry has no refusals among these (a hint it has no kernel for runs the nearest tile: dy rows that are not 16-byte addressable
    and merge_x take the 64x64 tile).  DENSE loader: the dense 1x1 cases; decoding loader: everything else, `pwgap` being the 1x1
    that a batch-stride gap makes non-dense."""
    L, ops = X
    cd = R.case_data(name)
    t = Tally()
    side = WgSide(cd)
    for v in WG_VARIANTS:
        for acc in (0, 1):
            run_wgrad(L, L.lib.zsg_conv_wgrad, side, wg_hint(v), acc, t, f"{name} wgrad variant {v} accumulate {acc}")
    t.report(f"zsg_conv_wgrad {name}")


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASE[n].wino])
def test_wgrad_wino_exact(X, name):
    """zsg_conv_wgrad_wino: splits 0 / 1 / 2 / 4, both block orders, accumulate, the channel window; zsg_conv_wgrad_wino_batched with
    2 and 8 jobs (odd jobs get -dy: their gradient is the negated one, so a job that reads another job's operands is seen)"""
    L, ops = X
    cd = R.case_data(name)
    c = cd.c
    t = Tally()
    side = WgSide(cd)
    for sp in (0, 1, 2, 4):
        for xmap in (0, 1):
            for acc in (0, 1):
                run_wgrad(L, L.lib.zsg_conv_wgrad_wino, side, (sp << 16) | (xmap << 24), acc, t, f"{name} wgrad_wino splits {sp} order {xmap} accumulate {acc}")
    neg = Dev(side.dy.buf, -side.dy.t)
    exp_neg = {}
    for acc in (0, 1):
        ref = torch.zeros(R.wt_extent(cd.W), dtype=R.DT)
        ref[cd.w_idx] = -cd.dw() + (cd.dw_prev if acc else 0)
        exp_neg[acc] = R.expected_output(side.init[acc].buf, ref, cd.w_idx.reshape(-1)).cuda()
    for J in (2, 8):
        for sp, xmap, acc in ((0, 0, 0), (1, 0, 1), (2, 1, 0), (4, 0, 1)):
            d = cdesc(L, cd.W, (sp << 16) | (xmap << 24))
            dws = [side.init[acc].clone() for _ in range(J)]
            arr = lambda ps: (C.c_void_p * J)(*ps)
            rc = L.lib.zsg_conv_wgrad_wino_batched(C.byref(d), J, arr([side.src.ptr] * J), arr([(neg if j & 1 else side.dy).ptr for j in range(J)]),
                                                   arr([w.ptr for w in dws]), acc, WS.data_ptr(), WS.numel() * 4, L.stream_ptr())
            assert rc == 0, L.lib.zsg_last_error().decode()
            for j, w in enumerate(dws):
                same(f"{name} wgrad_wino_batched J {J} job {j} splits {sp} order {xmap} accumulate {acc}", w, (exp_neg if j & 1 else side.exp)[acc])
            t.ran += 1
    t.report(f"zsg_conv_wgrad_wino + batched {name}")


@pytest.mark.parametrize("name", ["n45", "pyr45"])
def test_wgrad_scalar_dy_rows(X, name):
    """dy rows that are not 16-byte addressable (N = 45 in 45-wide rows, the [B, P, 45] scatter): zsg_conv_wgrad's scalar-load variant,
    whatever the hint asks for"""
    L, ops = X
    cd = R.case_data(name)
    c = cd.c
    W = R.fwd_desc(c.src_view(), c.out_view(45), c.C, c.N, c.k, c.s, c.p, c.d, c.wC, c.wc0, c.wt_ld)
    assert W.out_ld == 45
    t = Tally()
    side = WgSide(cd, W)
    for v in WG_VARIANTS:
        for acc in (0, 1):
            run_wgrad(L, L.lib.zsg_conv_wgrad, side, wg_hint(v), acc, t, f"{name} wgrad, dy in 45-wide rows, variant {v} accumulate {acc}")
    t.report(f"zsg_conv_wgrad {name} (dy rows of 45)")


def _wide_case(gap_short):
    """a 3x3 convolution over two small images whose IMAGE STRIDE is 2^23 elements (the 32-bit-multiply fallback of zsg_conv_wgrad) or
    four elements less (the last stride the 24-bit multiplies serve)"""
    h, w, ld = 6, 5, 16
    return R.Case("wide", 2, 16, 32, [(h, w)], 3, 1, 1, src_gap=(1 << 23) - gap_short - h * w * ld)


@pytest.mark.parametrize("short", [0, 4], ids=["stride_2p23", "stride_below"])
def test_wgrad_image_stride_limit(X, short):
    L, ops = X
    c = _wide_case(short)
    assert c.src_view().levels[0].bstride == (1 << 23) - short
    cd = R.CaseData(c)
    t = Tally()
    side = WgSide(cd)
    for v in (0, (64, 64, 1, 0, 0), (128, 128, 2, 1, 1), (64, 128, 3, 0, 0)):
        for acc in (0, 1):
            run_wgrad(L, L.lib.zsg_conv_wgrad, side, wg_hint(v), acc, t, f"image stride 2^23 - {short}: wgrad variant {v} accumulate {acc}")
    t.report(f"zsg_conv_wgrad image stride 2^23 - {short}")


@pytest.mark.parametrize("name", ["c3", "n45", "c36", "pw722", "stem"])
def test_transpose_w_exact(X, name):
    """zsg_transpose_w and zsg_transpose_w_batched: dst[c][t][n] = src[n][t][c], pad columns N..dst_ld-1 zeroed, nothing else touched"""
    L, ops = X
    cd = R.case_data(name)
    c = cd.c
    T = c.k * c.k
    n_el = c.N * T * c.C
    src = Dev(R.build_input(n_el, torch.arange(n_el), cd.w_dense.reshape(-1)))
    dst_n = c.C * T * c.dy_ld
    ref = cd.wt.reshape(-1)
    dst = Dev(R.build_output(dst_n, torch.arange(dst_n)))
    exp = R.expected_output(dst.buf, ref, torch.arange(dst_n)).cuda()
    L.check(L.lib.zsg_transpose_w(src.ptr, dst.ptr, c.N, T, c.C, c.dy_ld, L.stream_ptr()), "transpose_w")
    same(f"{name}: zsg_transpose_w", dst, exp)
    # two jobs in one launch, the second image GUARD elements behind the first
    two = Dev(R.build_output(2 * dst_n + R.GUARD, torch.cat([torch.arange(dst_n), dst_n + R.GUARD + torch.arange(dst_n)])))
    tc, tn = (c.C + 63) // 64, (c.dy_ld + 63) // 64
    jobs = b"".join(struct.pack("<qqiiiiiiii", 0, j * (dst_n + R.GUARD), c.N, T, c.C, c.dy_ld, j * T * tc * tn, tc, tn, 0) for j in range(2))
    jd = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).cuda()
    L.check(L.lib.zsg_transpose_w_batched(src.ptr, two.ptr, jd.data_ptr(), 2, 2 * T * tc * tn, L.stream_ptr()), "transpose_w_batched")
    ref2 = torch.zeros(2 * dst_n + R.GUARD, dtype=R.DT)
    ref2[:dst_n] = ref
    ref2[dst_n + R.GUARD:] = ref
    same(f"{name}: zsg_transpose_w_batched", two, R.expected_output(two.buf, ref2, torch.cat([torch.arange(dst_n), dst_n + R.GUARD + torch.arange(dst_n)])).cuda())


def test_negative_control_neighbouring_geometry(X):
    """the comparison CAN fail: the result of `c3` (pad 1) against the reference of the neighbouring geometry (pad 0 on the same grid)"""
    L, ops = X
    cd = R.case_data("c3")
    side = fwd_side(cd)
    init, exp, *_ = side.epi("plain")
    out = init.clone()
    L.check(L.lib.zsg_conv_igemm(C.byref(cdesc(L, cd.F)), side.src.ptr, side.wt.ptr, out.ptr, None, None, None, None, L.stream_ptr()), "igemm")
    assert torch.equal(out.t, exp)
    ref = torch.zeros(R.out_extent(cd.F), dtype=R.DT)
    ref[R.out_index(cd.F, 0)] = R.pad0_neighbour_rows(cd)[0]
    wrong = R.expected_output(init.buf, ref, side.written).cuda()
    assert not torch.equal(out.t, wrong)
    with pytest.raises(AssertionError, match="GEMM row"):
        same("negative control", out, wrong, cd.F)


def test_every_variant_runs_somewhere():
    """no silent skips: every listed variant is accepted (expected_rc == 0, which the per-case tests hold the library to) on at least
    one case, every variant of the refusal lists on none, and every case accepts hint 0"""
    sides = [(c.name, c.fwd(), c.out_shift != 0) for c in R.CASES]
    for v in IG_VARIANTS:
        assert any(expected_rc(D, v, "plain", u) == 0 for _, D, u in sides), f"igemm variant {v} runs on no case"
    for v in IG_REFUSED:
        assert all(expected_rc(D, v, "plain", u) == -1 for _, D, u in sides if not D.merge_x or v[5] or v[0] == 32), f"igemm variant {v} is in the refusal list"
    for epi in EPIS:
        assert any(expected_rc(D, (64, 64, 0, 0, 1, 0), epi, u) == 0 for _, D, u in sides)
    wn = [(c.fwd(), c.out_shift != 0) for c in R.CASES if c.wino]
    for v in WN_VARIANTS:
        assert any(expected_rc_wino(D, v, "plain", u) == 0 for D, u in wn), f"wino variant {v} runs on no case"
    for v in WN_REFUSED:
        assert all(expected_rc_wino(D, v, "plain", u) == -1 for D, u in wn)
    assert all(expected_rc(D, None, "plain", u) == 0 for _, D, u in sides)
    for uw in (32, 64, 128):
        assert any(pw_ok(c.fwd(), uw) for c in R.CASES), f"the streaming 1x1 kernel's unit width {uw} runs on no case"
    # the streaming kernels: pw on the dense 1x1 cases, mx on the stem cases, and a 1x1 they must refuse (a batch-stride gap)
    assert pw_ok(R.CASE["pw722"].fwd(), 64) and not pw_ok(R.CASE["pwgap"].fwd(), 64) and not pw_ok(R.CASE["pad8"].fwd(), 64)
    assert mx_ok(R.CASE["stem"].fwd()) and mx_ok(R.CASE["stem3"].fwd())


# ---- the tuner offers nothing that is not exactness-tested ---------------------------------------------------------------------------
def _decode_ig(h):
    return (h & 0xff, (h >> 8) & 0xff, (h >> 24) & 1, (h >> 27) & 1, max(1, (h >> 16) & 0xff), (h >> 28) & 3)


def _decode_wn(h):
    return (h & 0xff, (h >> 8) & 0xff, (h >> 24) & 1, max(1, (h >> 16) & 0xff), (h >> 28) & 3)


@pytest.mark.parametrize("name", [n for n in NAMES if len(R.CASE[n].sizes) == 1])
def test_tuner_candidates_are_exact(X, name, monkeypatch):
    """every tile hint ops.autotune_conv offers for the case's forward, data gradient and weight gradient (Winograd ones included) is
    either one of the variants the tests above RUN on this geometry (in the static lists and accepted here: expected_rc == 0) or is
    launched here, against the same references; a data gradient's candidates are launched here with the accumulate + mask epilogue the
    training plans give them as well.  A candidate the library refuses (the tuner may offer one: it drops what the warm-up launch
    refuses) is launched here too, must be refused as predicted, and is counted apart.  The tuner's
    state is put back afterwards, and it registers no stream-K scratch of its own: this module's stream has one (fixture X), and the
    default stream's registration — which test_gpu_streamk.py inspects — is not touched."""
    L, ops = X
    cd = R.case_data(name)
    c = cd.c
    saved = (dict(ops._TUNE_CACHE), dict(ops._TUNE_ALTS), ops._TUNE_DIRTY, dict(ops.TUNE_INFO))
    offered = []

    def record(trials, set_hint, stream, penalty):
        offered.extend((t[0], t[2], t[3]) for t in trials)
        return trials[0][2] | trials[0][3]
    monkeypatch.setattr(ops, "_pick_best", record)
    monkeypatch.setattr(ops, "ensure_stream_scratch", lambda stream: None)
    view = lambda dv: dv.t[dv.buf.lo:]
    t = Tally()
    known = extra = off_refused = 0
    try:
        ops._TUNE_CACHE.clear()
        st = L.stream_ptr()
        sides = [(fwd_side(cd, c.out_shift), True)] + ([] if c.merge_x else [(dg_side(cd), False)])
        for side, is_fwd in sides:
            offered.clear()
            init = side.epi("plain")[0].clone()
            U = wargs = None
            if c.wino:
                if is_fwd:
                    U, _ = make_u(L, ops, side.wt.ptr + 4 * c.wc0, c.N, c.C, c.wt_ld, c.wC, False)
                else:
                    U, _ = make_u(L, ops, side.wt.ptr, c.C, c.dy_ld, 9 * c.dy_ld, c.dy_ld, True)
                wargs = (view(side.src), view(U), view(init), None, None, None, None)
            ops.autotune_conv("igemm", L.lib.zsg_conv_igemm, cdesc(L, side.D), (view(side.src), view(side.wt), view(init), None, None, None, None),
                              st, wino_args=wargs, allow_sk=is_fwd)
            assert offered, "the tuner offered nothing"
            for fn, h, flag in list(offered):
                what = f"{name} {'forward' if is_fwd else 'dgrad'} tuner candidate {hex(h | flag)}"
                if flag:
                    v, fn_, wp, rcf, lst, sp = _decode_wn(h), L.lib.zsg_conv_wino, U.ptr, expected_rc_wino, WN_VARIANTS, _decode_wn(h)[3]
                    assert wn_hint(v) == h, what
                else:
                    v, fn_, wp, rcf, lst, sp = _decode_ig(h), L.lib.zsg_conv_igemm, side.wt.ptr, expected_rc, IG_VARIANTS, _decode_ig(h)[4]
                    assert ig_hint(v) == h, what
                want = rcf(side.D, v, "plain", c.out_shift != 0)
                off_refused += want != 0
                if v in lst and want == 0:
                    known += 1
                else:
                    extra += 1
                    run_fwd_entry(L, fn_, side, wp, h, "plain", want, t, what)
                if not is_fwd:
                    epi = "acc_mask_z" if sp > 1 else "acc_mask"
                    run_fwd_entry(L, fn_, side, wp, h, epi, rcf(side.D, v, epi, False), t, f"{what} {epi}")
        # the weight gradient (and its Winograd form)
        offered.clear()
        wside = WgSide(cd)
        dw = wside.init[0].clone()
        wst = WS._get()
        a = (view(wside.src), view(wside.dy), view(dw), 0, wst, wst.numel() * 4)
        ops.autotune_conv("wgrad", L.lib.zsg_conv_wgrad, cdesc(L, cd.W), a, st, ws_bytes=wst.numel() * 4, wino_args=a if c.wino else None)
        assert offered
        wg_known = {wg_hint(v) for v in WG_VARIANTS}
        for fn, h, flag in list(offered):
            what = f"{name} wgrad tuner candidate {hex(h | flag)}"
            if flag:          # zsg_conv_wgrad_wino reads the split and block-order fields only
                isk = ((h >> 16) & 0xff) in (0, 1, 2, 4)
            else:
                isk = h in wg_known
            known += isk
            extra += not isk
            if not isk:
                run_wgrad(L, L.lib.zsg_conv_wgrad_wino if flag else L.lib.zsg_conv_wgrad, wside, h, 0, t, what)
    finally:
        ops._TUNE_CACHE.clear()
        ops._TUNE_CACHE.update(saved[0])
        ops._TUNE_ALTS.clear()
        ops._TUNE_ALTS.update(saved[1])
        ops._TUNE_DIRTY = saved[2]
        ops.TUNE_INFO.clear()
        ops.TUNE_INFO.update(saved[3])
    print(f"tuner {name}: {known + extra} candidates offered ({off_refused} of them the library refuses), {known} among the variants that "
          f"ran in the tests above, {extra} more launched here; with the data gradients' accumulate + mask replays {t.ran} launches compared "
          f"at zero tolerance, {t.refused} refused as expected")

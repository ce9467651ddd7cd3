"""Exact-arithmetic, guarded tests of the BatchNorm-fused convolution entries through the C ABI: zsg_conv_igemm_bnb / zsg_conv_wino_bnb
(BatchNorm-backward sums in the data gradient's epilogue, the streaming 1x1 kernel behind BM = 32 included), zsg_conv_igemm_bnstat /
zsg_conv_wino_bnstat / zsg_conv_igemm_bnb_tail / zsg_conv_wino_bnb_tail (the cross-workgroup finalize of csrc/bn_tail.h),
zsg_conv_igemm_bnpre (the BatchNorm-applying operand loader) and zsg_conv_bn_tail_tickets.

Method of tests/test_gpu_conv_exact.py: integer operands and power-of-two scales (tests/conv_bn_exact_ref.py; the bounds that make
every stored value, partial-row element and column total exact in fp32 are proved per case by tests/test_cpu_conv_bn_exact.py, which
also holds the reference to independent fp64 torch and shows that seven subtly wrong references are told apart).  Every buffer of a
launch — operands, out, partials, tickets, coef, mean, invstd, dgamma, dbeta, running statistics, pre_y, pre_relu_mask — sits between
guards; outputs hold NaN (0xAA for mask bytes) where the launch must write and sentinels elsewhere; the WHOLE buffers are compared,
operands included (they must come back unchanged).  Every accepted launch runs twice and must give identical bits.  Zero tolerance
(equality of the bit patterns) for the stored output (the epi_flags form too), every partial row of the implicit-GEMM and Winograd
tiles, the streaming kernel's column totals and row count, dgamma, dbeta, pre_y, every pre_relu_mask byte and the tickets (zero after
the launch); mean / invstd / coef / running statistics pass an fp64 division or square root on the device and must lie within 1 fp32
ulp of the fp64 reference — bit-equal for mean / coef where n is a power of two — and the tests print how many elements differed by
that ulp.  The fused launch stores the bits of the plain zsg_conv_igemm / zsg_conv_wino launch with the same hint.  A refusal returns
-1, names its entry in zsg_last_error, leaves every byte of every buffer as it was, and zsg_conv_bn_tail_tickets says -1 for the
same descriptor where the descriptor is the reason.

Where each gap of the older files (test_gpu_bnb.py, test_gpu_bntail.py, test_gpu_ops.py::test_conv_igemm_bnpre) is closed:

    kernel path                      edge                                                        test [case]
    igemm / wino epilogue + reduce   one row tile (reducer waits for 0 arrivals), rows == 1      test_bnb_exact / test_bnstat_exact [d_m1, f_m1, d_w1, f_w1], test_bnpre_exact [p_m1]
    igemm epilogue                   a row tile holding a single row (M = 65 at BM = 64)         test_bnb_exact [d_m65, d_n132], test_bnstat_exact [f_m65], test_bnpre_exact [p_m65]
    bn_tail_reduce                   exactly 128 partial rows per column block                   test_row_limit [r128 (BM 64), r128b (BM 128)]
    conv_*_impl, tickets             129 partial rows: refused, tickets -1                       test_row_limit [r129, r129b]
    epilogue, reduce column groups   N = 68 / 132 / 36: a last column block of 4 channels        [d_m65, f_m65, p_m65; d_n132, f_n132, p_m722; d_w1, d_w5, f_w1, f_w5]
    K loop                           K = 36, 40 (no multiple of 32)                              [d_m65, d_m722, d_w5, d_w107, f_*]
    finalize over segments           nseg = 4 with the finalize (rows summed over segments)      test_bnb_exact [d_pyr, d_s2], test_bnstat_exact [f_pyr]
    stream-K + sums / finalize       fewer tiles than workgroups: 2 tiles K = 1024, K = 32       [d_sk1024, d_sk32, f_sk1024, f_sk32] (and every small case: 1 - 24 tiles)
    bn_tail_reduce mode 1            accumulate == 0 and 1 for dgamma / dbeta                    test_bnb_exact (every case, forms of TAIL_FORMS)
    argument forms                   running_* NULL, bn_relu_mask NULL, pre_relu_mask NULL,      test_bnstat_exact, test_bnb_exact, test_bnpre_exact (forms)
                                     bn_partials NULL, tickets NULL, add_src NULL / separate / aliasing out, epi_flags 0 / 1
    streaming 1x1 kernel (pw.hip)    unit widths 32 / 64 / 128 at M = 1, 33, 722, K = 64, 128    test_bnb_exact [d_pw1, d_pw33n (four panels), d_pw722]
                                     K = 512: width 32 (64 / 128 fit no LDS panel: refused)      test_bnb_exact [d_pw33, d_pw722k]
    Winograd tiles                   TB, BN in {32, 64}, position-group bit, its stream-K bit,   test_bnb_exact / test_bnstat_exact [d_w*, f_w*, d_n132, d_pyr]
                                     1x1, 3x3, 5x5, 10x7, 19x19 maps (overhang pixels)
    taps                             3x3 stride 2 (four parity segments), dilation 6             [d_s2, d_dil6, f_dil6]
    guards                           every buffer guarded, whole buffers compared                every test
    refusals, nothing written        _bnb: split-K, N % 4, out_off % 4, bn_x unaligned,          test_bnb_refusals
                                     merge_x, NULL partials
                                     finalize: hint 0, BM = 32, split-K, NULL tickets/coef/mean  test_finalize_refusals (129 rows: test_row_limit)
                                     _bnpre: C = 48, 3x3, strided, non-dense source, wc0, 64-deep test_bnpre_refusals
                                     K, 4-wave 128x128, BM = 32, relu = 1, unaligned pre_*

Not tested, on purpose: the bounded poll's time-out / poison path and non-zero tickets at entry (reaching either means making a launch
wait); the caller obligation "every output element covered by the launch" (a zero_fill descriptor) stays a documented contract."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_bn_exact_ref as B  # noqa: E402
import conv_exact_ref as R  # noqa: E402
from test_gpu_conv_exact import NUM_CU, SK_FORMS, TILES, X, cdesc, ig_hint, make_u, pw_ok, refusal_message, stale_error, wn_hint  # noqa: E402,F401
from test_gpu_ops import Z  # noqa: E402,F401

G = R.GUARD
TICKET_GUARD = 0x5A5A5A5A


# ---- guarded device buffers -----------------------------------------------------------------------------------------------------------
class Gb:
    """a device buffer [guard | n elements | guard]; ptr = the first element behind the front guard"""

    def __init__(self, t, lo, n, null=False):
        self.t, self.lo, self.n, self.null = t, lo, n, null          # null: the launch is handed NULL for this buffer

    @property
    def ptr(self):
        return None if self.null else self.t.data_ptr() + self.lo * self.t.element_size()

    @property
    def body(self):
        return self.t[self.lo:self.lo + self.n]

    def clone(self):
        return Gb(self.t.clone(), self.lo, self.n, self.null)


def g_in(vals, idx=None, extent=None, shift=0):
    """a float operand: NaN guards; with idx / extent: poison wherever the descriptor does not address"""
    vals = vals.reshape(-1)
    n = len(vals) if extent is None else extent
    b = R.build_input(n, torch.arange(n) if idx is None else idx, vals, shift)
    return Gb(b.t.cuda(), b.lo, n)


def g_out(n, init=None):
    """a float output: sentinel guards, NaN (or `init`) where the launch must write"""
    b = R.build_output(n, torch.arange(n), init)
    return Gb(b.t.cuda(), b.lo, n)


def g_bytes(body=None, n=None):
    """mask bytes between 0x55 guards; an output holds 0xAA"""
    n = len(body) if body is not None else n
    t = torch.full((G + n + G,), 0x55, dtype=torch.uint8)
    t[G:G + n] = 0xAA if body is None else body
    return Gb(t.cuda(), G, n)


def g_tickets(n):
    t = torch.full((G + n + G,), TICKET_GUARD, dtype=torch.int32)
    t[G:G + n] = 0
    return Gb(t.cuda(), G, n)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def filled(g: Gb, ref):
    """the complete buffer a correct launch leaves: g with its body replaced by the reference"""
    e = g.t.clone()
    e[g.lo:g.lo + g.n] = ref.reshape(-1).to(e.dtype)
    return e


def differs(what, name, got: Gb, exp):
    a, b = bits(got.t).cpu(), bits(exp).cpu()
    bad = (a != b).nonzero().view(-1)
    i = int(bad[0])
    where = " — inside a guard" if i < got.lo or i >= got.lo + got.n else ""
    return (f"{what}: {name}: {len(bad)} of {a.numel()} elements differ; first at buffer index {i} (element {i - got.lo}): "
            f"got {got.t[i].item()!r}, want {exp[i].item()!r}{where}")


class Tally:
    def __init__(self):
        self.ran = self.refused = 0
        self.ulp = {}

    def count(self, name, d):
        a, b = self.ulp.get(name, (0, 0))
        self.ulp[name] = (a + int((d == 1).sum()), b + d.numel())

    def report(self, what):
        u = ", ".join(f"{k} {a}/{b}" for k, (a, b) in sorted(self.ulp.items()))
        print(f"{what}: {self.ran} launches compared (every buffer whole, each run twice), {self.refused} refused with nothing written"
              + (f"; elements 1 ulp off the fp64 reference: {u}" if u else ""))


def run(L, what, call, bufs, expect, ulp, want, word, T: Tally, tickets_say=None, custom=None):
    """one launch configuration: `bufs` name -> Gb is the pre-launch state, call(b) launches on clones b.  Accepted: every buffer named in
    `expect` equals the given complete buffer bit for bit, every one in `ulp` (name -> (fp64 reference, exact)) keeps its guards and
    lies within 1 ulp (exact: 0), one in `custom` passes its own check, every other buffer is unchanged; a second run gives identical
    bits.  Refused: rc -1, the message names the entry, every buffer unchanged, and tickets_say (zsg_conv_bn_tail_tickets for a
    descriptor that is itself the reason) is -1.  Returns the first run's buffers (None: refused)."""
    custom = custom or {}
    first = None
    for rep in range(2):
        b = {k: v.clone() for k, v in bufs.items()}
        stale = stale_error(L) if want else None
        rc = call(b)
        assert rc == want, f"{what}: return code {rc}, expected {want} ({L.lib.zsg_last_error().decode()})"
        if rc:
            assert word in refusal_message(L, stale, what), f"{what}: zsg_last_error must name the entry ({L.lib.zsg_last_error().decode()})"
            for k, g in b.items():
                assert torch.equal(bits(g.t), bits(bufs[k].t)), differs(what + ": refused, yet written", k, g, bufs[k].t)
            if tickets_say is not None:
                assert tickets_say == -1, f"{what}: zsg_conv_bn_tail_tickets says {tickets_say} for a descriptor the entry refuses"
            T.refused += 1
            return None
        for k, g in b.items():
            if k in expect:
                assert torch.equal(bits(g.t), bits(expect[k])), differs(what, k, g, expect[k])
            elif k in custom:
                custom[k](g, bufs[k])
            elif k in ulp:
                ref, exact = ulp[k]
                e = filled(bufs[k], ref)
                body = torch.zeros_like(g.t, dtype=torch.bool)
                body[g.lo:g.lo + g.n] = True
                assert torch.equal(bits(g.t)[~body], bits(e)[~body]), differs(what + " (guards)", k, g, e)
                got = g.body.cpu()
                assert not torch.isnan(got).any(), f"{what}: {k}: NaN (not written, or poisoned)"
                d = (got.view(torch.int32).long() - e[g.lo:g.lo + g.n].cpu().view(torch.int32).long()).abs()
                if first is None:
                    T.count(k, d)
                assert int(d.max()) <= (0 if exact else 1), (f"{what}: {k}: {int((d > 0).sum())} of {d.numel()} elements off the fp64 reference, worst {int(d.max())} ulp "
                                                               f"(allowed {0 if exact else 1}); first: got {float(got[int(d.argmax())])!r}, want {float(ref.reshape(-1)[int(d.argmax())])!r}")
            else:
                assert torch.equal(bits(g.t), bits(bufs[k].t)), differs(what + ": must stay unchanged", k, g, bufs[k].t)
        if first is None:
            first = b
        else:
            for k in b:
                assert torch.equal(bits(b[k].t), bits(first[k].t)), f"{what}: {k}: two runs differ"
    T.ran += 1
    return first


def p_(g):
    return None if g is None else g.ptr


# ---- variants -------------------------------------------------------------------------------------------------------------------------
IG_V = ([(bm, bn, w8, k64, 1, 0) for bm, bn in TILES for w8 in (0, 1) for k64 in (0, 1)]
        + [f + (1, sk) for f in SK_FORMS for sk in (1, 2)]
        + [(32, 32, 0, 0, 1, 0), (32, 64, 0, 0, 1, 0), (32, 128, 0, 0, 1, 0)])
WN_V = [(tb, bn, ps4, 1, 0) for tb in (32, 64) for bn in (32, 64) for ps4 in (0, 1)] + [(32, 64, 1, 1, 1)]
IG_FEW = [(64, 64, 0, 0, 1, 0), (128, 64, 1, 0, 1, 0), (128, 128, 0, 0, 1, 0)]          # the 4 MB geometries of the row-count limit
PRE_V = [(64, 64, 0, 0, 1, 0), (64, 64, 1, 0, 1, 0), (128, 64, 0, 0, 1, 0), (128, 64, 1, 0, 1, 0), (128, 128, 1, 0, 1, 0)]


def row_tiles(D, bm):
    return sum(-(-D.B * g.rows_y * g.rows_x // bm) for g in D.segs)


def wino_blocks(D, tb):
    return sum(-(-D.B * ((g.src_H + 1) // 2) * ((g.src_W + 1) // 2) // tb) for g in D.segs)


def ig_rc(D, v, tail):
    """include/zsg.h: tiles 64x64 / 128x64 / 128x128, no split-K; stream-K: one segment, the six forms, fewer tiles than workgroups;
    BM = 32: the streaming 1x1 kernel's geometries, no in-kernel finalize; the finalize: at most 128 partial rows per column block"""
    bm, bn, w8, k64, sp, sk = v
    if bm == 32:
        return 0 if pw_ok(D, bn) and not tail and not sk and sp <= 1 else -1
    if (bm, bn) not in TILES or sp > 1:
        return -1
    mt = row_tiles(D, bm)
    if sk and (D.nseg != 1 or (bm, bn, w8, k64) not in SK_FORMS or mt * -(-D.N // bn) > NUM_CU * sk):
        return -1
    return -1 if tail and mt > 128 else 0


def wn_rc(D, v, tail):
    tb, bn, ps4, sp, sk = v
    if tb not in (32, 64) or bn not in (32, 64) or sp > 1:
        return -1
    mb = wino_blocks(D, tb)
    if sk and (D.nseg != 1 or (tb, bn, ps4) != (32, 64, 1) or mb * -(-D.N // bn) > NUM_CU):
        return -1
    return -1 if tail and mb > 128 else 0


def hint_of(kern, v):
    return wn_hint(v) if kern == "wn" else ig_hint(v)


def desc_of(L, D, kern, v, epi=0):
    d = cdesc(L, D, hint_of(kern, v) if v is not None else 0, D.relu)
    d.epi_flags = epi
    return d


def pow2(n):
    return n & (n - 1) == 0


# ---- operands of a case on the device -------------------------------------------------------------------------------------------------
class Side:
    def __init__(self, L, ops, bd):
        self.bd, self.D = bd, bd.D
        D, c = bd.D, bd.c
        self.N, self.ext, self.n = c.N, bd.ext, B.total_rows(D)
        self.wt = g_in(bd.w)
        if c.mode == "pre":
            self.src = g_in(bd.x)
            self.pre = {k: g_in(getattr(bd, "pre_" + k)) for k in ("mean", "invstd", "gamma", "beta", "res")}
        else:
            self.src = g_in(bd.x[bd.x_idx], bd.x_idx, R.src_extent(D))
        if c.mode == "dg":
            self.bn_x, self.mean, self.invstd, self.add = g_in(bd.bn_x), g_in(bd.mean), g_in(bd.invstd), g_in(bd.add)
            self.mask = g_bytes(B.pack_bits(bd.bits))
        self.U = None
        if c.wino:          # the transformed filter image (of the rotated filter for a data gradient): exactness-tested by test_gpu_conv_exact.py
            u, self._jobs = make_u(L, ops, self.wt.ptr, D.N, D.C, 9 * D.C, D.C, c.mode == "dg")
            self.U = Gb(u.t, u.buf.lo, u.buf.extent)
        self.rm, self.rv = g_out(self.N, bd.rm0), g_out(self.N, bd.rv0)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def wptr(self, kern):
        return self.U.ptr if kern == "wn" else self.wt.ptr

    def out_init(self, alias_add=False):
        return self.memo(("oi", alias_add), lambda: g_out(self.ext, self.bd.add if alias_add else None))

    def part_rows(self, L, kern, v):
        if kern == "wn":
            return wino_blocks(self.D, v[0])
        rows = int(L.lib.zsg_conv_igemm_partial_rows(C.byref(desc_of(L, self.D, kern, v))))
        if v[0] != 32:
            assert rows == row_tiles(self.D, v[0]), f"zsg_conv_igemm_partial_rows {rows}, the layout has {row_tiles(self.D, v[0])}"
        return rows


def totals_check(what, prow, N, ref_tot):
    """the streaming kernel: one partial row per workgroup, no documented row assignment — the column totals over the
    zsg_conv_igemm_partial_rows rows are the contract, every promised row written, the guards untouched"""
    def check(got: Gb, init: Gb):
        inner = torch.zeros_like(got.t, dtype=torch.bool)
        inner[got.lo:got.lo + got.n] = True
        assert torch.equal(bits(got.t)[~inner], bits(init.t)[~inner]), f"{what}: the partial rows' guards"
        body = got.body.view(prow, 2, N)
        assert not torch.isnan(body).any(), f"{what}: a partial row of the promised {prow} was not written"
        assert torch.equal(body.double().sum(0).cpu(), ref_tot), f"{what}: column totals of the partial rows"
    return check


def tickets_must_say_no(D, kern, v):
    """include/zsg.h, zsg_conv_bn_tail_tickets: -1 without a hint, for the streaming 1x1 kernel, split-K, merge_x, more than 128 partial
    rows per column block (and output rows that are not 16-byte addressable, which the finalize's epilogue needs)"""
    if v is None or D.merge_x or D.N % 4 or D.out_ld % 4 or any(g.out_off % 4 or g.out_bstride % 4 for g in D.segs):
        return True
    if kern == "wn":
        return v[3] > 1 or wino_blocks(D, v[0]) > 128
    return v[0] == 32 or v[4] > 1 or row_tiles(D, v[0]) > 128


# ---- bnb / bnb_tail -------------------------------------------------------------------------------------------------------------------
BNB_FORMS = [dict(mask=1, add="alias", epi=0), dict(mask=1, add="sep", epi=1), dict(mask=0, add="none", epi=0), dict(mask=1, add="none", epi=0)]
TAIL_FORMS = [dict(mask=1, add="alias", epi=0, acc=1), dict(mask=1, add="none", epi=1, acc=0), dict(mask=0, add="sep", epi=0, acc=0)]


def bnb_launch(L, side: Side, kern, v, form, tail, T, what, want=None, plain_check=True):
    bd, D, N = side.bd, side.D, side.N
    want = (wn_rc if kern == "wn" else ig_rc)(D, v, tail) if want is None else want
    d = desc_of(L, D, kern, v, form["epi"])
    stream = v is not None and kern == "ig" and v[0] == 32
    prow = side.part_rows(L, kern, v) if v is not None else 1
    alias, has_add = form["add"] == "alias", form["add"] != "none"
    bufs = {"src": side.src, "wt": side.U if kern == "wn" else side.wt, "out": side.out_init(alias), "bn_x": side.bn_x, "mean": side.mean,
            "invstd": side.invstd, "mask": side.mask, "add": side.add, "part": side.memo(("pb", max(prow, 1)), lambda: g_out(max(prow, 1) * 2 * N))}
    nt = int(L.lib.zsg_conv_bn_tail_tickets(C.byref(d), 1 if kern == "wn" else 0))
    if tail:
        bufs["tickets"] = side.memo(("tk", max(nt, 1)), lambda: g_tickets(max(nt, 1)))
        bufs["coef"] = side.memo("coef", lambda: g_out(2 * N))
        for k, v0 in (("dgamma", bd.dg0), ("dbeta", bd.db0)):
            bufs[k] = side.memo((k, form["acc"]), lambda: g_out(N, v0 if form["acc"] else None))
    expect, ulp = {}, {}
    if want == 0:
        tile = None if stream else v[0]
        out, part = bd.bnb(tile, kern == "wn", bool(form["mask"]), has_add, form["epi"])
        expect["out"] = side.memo(("oe", form["add"], form["epi"], bool(form["mask"])), lambda: filled(bufs["out"], out))
        if not stream:
            assert part.shape[0] == prow
            expect["part"] = side.memo(("pe", tile, kern, form["mask"], has_add), lambda: filled(bufs["part"], part))
        if tail:
            assert nt == -(-N // v[1]), f"{what}: zsg_conv_bn_tail_tickets {nt}"
            fin = B.finalize_bwd(part[:, 0].sum(0), part[:, 1].sum(0), float(side.n), form["acc"], bd.dg0, bd.db0)
            expect["tickets"] = bufs["tickets"].t
            expect["dgamma"], expect["dbeta"] = filled(bufs["dgamma"], fin["dgamma"]), filled(bufs["dbeta"], fin["dbeta"])
            ulp["coef"] = (fin["coef"], pow2(side.n))
    fn = {("ig", 0): L.lib.zsg_conv_igemm_bnb, ("wn", 0): L.lib.zsg_conv_wino_bnb, ("ig", 1): L.lib.zsg_conv_igemm_bnb_tail,
          ("wn", 1): L.lib.zsg_conv_wino_bnb_tail}[(kern, int(tail))]
    st = L.stream_ptr()

    def call(b):
        a = (C.byref(d), b["src"].ptr, b["wt"].ptr, b["out"].ptr, b["out"].ptr if alias else (b["add"].ptr if has_add else None), b["bn_x"].ptr,
             b["mean"].ptr, b["invstd"].ptr, b["mask"].ptr if form["mask"] else None, b["part"].ptr)
        if tail:
            return fn(*a, b["tickets"].ptr, b["coef"].ptr, b["dgamma"].ptr, b["dbeta"].ptr, form["acc"], st)
        return fn(*a, st)
    custom = {}
    if stream and want == 0:
        custom["part"] = totals_check(what, prow, N, bd.bnb(None, False, bool(form["mask"]), has_add, form["epi"])[1][0])
    got = run(L, what, call, bufs, expect, ulp, want, "conv", T, nt if tail and tickets_must_say_no(D, kern, v) else None, custom)
    if got is not None and plain_check and not form["epi"]:
        plain = bufs["out"].clone()
        pf = L.lib.zsg_conv_wino if kern == "wn" else L.lib.zsg_conv_igemm
        L.check(pf(C.byref(desc_of(L, D, kern, v)), side.src.ptr, side.wptr(kern), plain.ptr, None, plain.ptr if alias else (side.add.ptr if has_add else None),
                   None, None, st), "the plain launch")
        assert torch.equal(bits(plain.t), bits(got["out"].t)), f"{what}: the fused launch must store the bits of the plain launch with the same hint"
    return got


DG = [c.name for c in B.CASES if c.mode == "dg" and not c.name.startswith("d_r1")]
FW = [c.name for c in B.CASES if c.mode == "fw" and not c.name.startswith("f_r1")]
PRE = [c.name for c in B.CASES if c.mode == "pre"]


@pytest.mark.parametrize("name", DG)
def test_bnb_exact(X, name):
    """zsg_conv_igemm_bnb / zsg_conv_wino_bnb and their *_tail forms on every tile variant the entries accept for the geometry (and
    refused, with nothing written, on the others)"""
    L, ops = X
    bd = B.data(name)
    side = Side(L, ops, bd)
    T = Tally()
    accepted = set()
    kinds = [("ig", v) for v in IG_V] + ([("wn", v) for v in WN_V] if bd.c.wino else [])
    for kern, v in kinds:
        for tail, forms in ((False, BNB_FORMS), (True, TAIL_FORMS)):
            for form in forms:
                if bnb_launch(L, side, kern, v, form, tail, T, f"{name} {kern} {v} {'tail ' if tail else ''}{form}") is not None:
                    accepted.add((kern, v[:4] if kern == "ig" else v[:3], tail))
    if name.startswith("d_pw"):
        # include/zsg.h: the filter panel must fit a CU's LDS — at K = 512 only panels of 32 channels do, whatever N is, so the unit
        # widths 64 and 128 exist at K = 64 / 128 only and are refused (pw_ok, as predicted) at K = 512
        widths = (32,) if bd.D.C == 512 else (32, 64, 128)
        assert {("ig", (32, uw, 0, 0), False) for uw in (32, 64, 128)} & accepted == {("ig", (32, uw, 0, 0), False) for uw in widths}, "the streaming kernel's unit widths"
    assert all(("ig", (bm, bn, w8, k64), t) in accepted for bm, bn in TILES for w8 in (0, 1) for k64 in (0, 1) for t in (False, True))
    if bd.D.nseg == 1:
        assert sum(1 for k, v in kinds if k == "ig" and v[5] and ig_rc(bd.D, v, True) == 0) == 12, "every stream-K form, with the finalize"
    if bd.c.wino:
        assert all(("wn", (tb, bn, ps4), t) in accepted for tb in (32, 64) for bn in (32, 64) for ps4 in (0, 1) for t in (False, True))
    T.report(f"bnb / bnb_tail {name} (M {side.n}, N {bd.c.N}, K {bd.D.C}, {bd.D.nseg} segments)")


# ---- bnstat ---------------------------------------------------------------------------------------------------------------------------
def stat_bufs(side: Side, prow, nt, running):
    N = side.N
    b = {"src": side.src, "out": side.out_init(), "part": side.memo(("pb", prow), lambda: g_out(prow * 2 * N)),
         "tickets": side.memo(("tk", max(nt, 1)), lambda: g_tickets(max(nt, 1))),
         "mean": side.memo("mo", lambda: g_out(N)), "invstd": side.memo("io", lambda: g_out(N))}
    if running:
        b["rm"], b["rv"] = side.rm, side.rv
    return b


def stat_expect(side: Side, bufs, tile, wino, running):
    bd = side.bd
    part = bd.stat(tile, wino)
    fin = B.finalize_fwd(part[:, 0].sum(0), part[:, 1].sum(0), float(side.n), bd.rm0, bd.rv0)
    expect = {"out": side.memo("oe", lambda: filled(bufs["out"], bd.out_flat())), "part": side.memo(("pe", tile, wino), lambda: filled(bufs["part"], part)),
              "tickets": bufs["tickets"].t}
    ulp = {"mean": (fin["mean"], pow2(side.n)), "invstd": (fin["invstd"], False)}
    if running:
        ulp["rm"], ulp["rv"] = (fin["rmean"], False), (fin["rvar"], False)
    return expect, ulp


def bnstat_launch(L, side: Side, kern, v, running, T, what, want=None):
    D, N = side.D, side.N
    want = (wn_rc if kern == "wn" else ig_rc)(D, v, True) if want is None else want
    d = desc_of(L, D, kern, v)
    prow = max(side.part_rows(L, kern, v), 1) if v is not None else 1
    nt = int(L.lib.zsg_conv_bn_tail_tickets(C.byref(d), 1 if kern == "wn" else 0))
    bufs = stat_bufs(side, prow, nt, running)
    bufs["wt"] = side.U if kern == "wn" else side.wt
    expect, ulp = stat_expect(side, bufs, v[0], kern == "wn", running) if want == 0 else ({}, {})
    if want == 0:
        assert nt == -(-N // v[1]), f"{what}: zsg_conv_bn_tail_tickets {nt}"
    fn = L.lib.zsg_conv_wino_bnstat if kern == "wn" else L.lib.zsg_conv_igemm_bnstat
    st = L.stream_ptr()

    def call(b):
        return fn(C.byref(d), b["src"].ptr, b["wt"].ptr, b["out"].ptr, b["part"].ptr, b["tickets"].ptr, b["mean"].ptr, b["invstd"].ptr,
                  b["rm"].ptr if running else None, b["rv"].ptr if running else None, B.MOM, 1e-5, st)
    got = run(L, what, call, bufs, expect, ulp, want, "conv", T, nt if tickets_must_say_no(D, kern, v) else None)
    if got is not None:
        plain, ppart = bufs["out"].clone(), bufs["part"].clone()
        pf = L.lib.zsg_conv_wino if kern == "wn" else L.lib.zsg_conv_igemm
        L.check(pf(C.byref(d), side.src.ptr, side.wptr(kern), plain.ptr, None, None, None, ppart.ptr, st), "the plain launch")
        assert torch.equal(bits(plain.t), bits(got["out"].t)) and torch.equal(bits(ppart.t), bits(got["part"].t)), \
            f"{what}: the same stored values and partial rows as the plain fused launch"
    return got


@pytest.mark.parametrize("name", FW)
def test_bnstat_exact(X, name):
    """zsg_conv_igemm_bnstat / zsg_conv_wino_bnstat: the forward statistics finalised in the launch, with and without running buffers"""
    L, ops = X
    bd = B.data(name)
    side = Side(L, ops, bd)
    T = Tally()
    ok = 0
    for kern, v in [("ig", v) for v in IG_V] + ([("wn", v) for v in WN_V] if bd.c.wino else []):
        for running in (True, False):
            ok += bnstat_launch(L, side, kern, v, running, T, f"{name} {kern} {v} running {running}") is not None
    assert ok >= 2 * (12 + (12 if bd.D.nseg == 1 else 0) + (8 if bd.c.wino else 0))
    T.report(f"bnstat {name} (M {side.n}, N {bd.c.N}, K {bd.D.C}, {bd.D.nseg} segments)")


# ---- the row-count limit of the finalize ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["r128", "r129", "r128b", "r129b"])
def test_row_limit(X, which):
    """exactly 128 partial rows per column block are reduced exactly; 129 make zsg_conv_bn_tail_tickets say -1 and the *_bnstat /
    *_bnb_tail entries refuse with nothing written (BM = 64: 2x64x64 / 1x86x96, BM = 128: 1x128x128 / 1x129x128; C = 32, N = 64)"""
    L, ops = X
    T = Tally()
    for mode in ("f_", "d_"):
        bd = B.data(mode + which)
        side = Side(L, ops, bd)
        seen = set()
        for v in IG_FEW:
            mt = row_tiles(bd.D, v[0])
            want = 0 if mt <= 128 else -1
            assert ig_rc(bd.D, v, True) == want
            seen.add(mt)
            nt = int(L.lib.zsg_conv_bn_tail_tickets(C.byref(desc_of(L, bd.D, "ig", v)), 0))
            assert nt == (1 if want == 0 else -1), (v, mt, nt)
            what = f"{mode}{which} {v} ({mt} partial rows)"
            if mode == "f_":
                bnstat_launch(L, side, "ig", v, True, T, what)
            else:
                bnb_launch(L, side, "ig", v, TAIL_FORMS[0], True, T, what, plain_check=False)
                if want:          # the entry without the finalize takes any number of rows
                    bnb_launch(L, side, "ig", v, BNB_FORMS[1], False, T, what + " without the finalize", plain_check=False)
        assert (128 if "128" in which else 129) in seen
    T.report(f"row-count limit {which}")


# ---- bnpre ----------------------------------------------------------------------------------------------------------------------------
PRE_FORMS = [dict(tk=1, part=1, mask=1, run=1), dict(tk=0, part=1, mask=1, run=0), dict(tk=0, part=0, mask=0, run=0), dict(tk=1, part=1, mask=0, run=0)]


def pre_launch(L, side: Side, v, form, T, what, want=0, D=None, tweak=None, word="conv_igemm"):
    bd, N = side.bd, side.N
    D = side.D if D is None else D
    Cc = bd.c.K
    d = desc_of(L, D, "ig", v)
    prow = row_tiles(side.D, v[0]) if v is not None and v[0] != 32 else 1
    nt = int(L.lib.zsg_conv_bn_tail_tickets(C.byref(d), 0))
    bufs = stat_bufs(side, prow, nt, form["run"])
    bufs["wt"] = side.wt
    bufs.update({"pre_" + k: g for k, g in side.pre.items()})
    bufs["pre_y"] = side.memo("py", lambda: g_out(side.n * Cc))
    bufs["pre_mask"] = side.memo("pm", lambda: g_bytes(n=side.n * Cc // 4))
    expect, ulp = {}, {}
    if want == 0:
        e2, u2 = stat_expect(side, bufs, v[0], False, form["run"])
        expect["out"] = e2["out"]
        expect["pre_y"] = side.memo("pye", lambda: filled(bufs["pre_y"], bd.pre_y))
        if form["mask"]:
            expect["pre_mask"] = side.memo("pme", lambda: filled(bufs["pre_mask"], B.pack_bits(bd.pre_bits)))
        if form["part"]:
            expect["part"] = e2["part"]
        if form["tk"]:
            assert nt == -(-N // v[1])
            expect["tickets"] = e2["tickets"]
            ulp = u2
    st = L.stream_ptr()

    def call(b):
        a = {k: b[k].ptr for k in b}
        if tweak:
            tweak(a)
        return L.lib.zsg_conv_igemm_bnpre(C.byref(d), a["src"], a["wt"], a["out"], a["part"] if form["part"] else None, a["tickets"] if form["tk"] else None,
                                          a["mean"], a["invstd"], a["rm"] if form["run"] else None, a["rv"] if form["run"] else None, B.MOM, 1e-5,
                                          a["pre_mean"], a["pre_invstd"], a["pre_gamma"], a["pre_beta"], a["pre_res"], a["pre_y"],
                                          a["pre_mask"] if form["mask"] else None, st)
    return run(L, what, call, bufs, expect, ulp, want, word, T)


@pytest.mark.parametrize("name", PRE)
def test_bnpre_exact(X, name):
    """zsg_conv_igemm_bnpre on every tile it accepts: the materialised activation, every ReLU-bit byte (exact zeros have bit 0), the
    convolution, its partial rows and their in-kernel finalize"""
    L, ops = X
    bd = B.data(name)
    side = Side(L, ops, bd)
    T = Tally()
    for v in PRE_V:
        for form in PRE_FORMS:
            pre_launch(L, side, v, form, T, f"{name} {v} {form}")
    assert T.ran == len(PRE_V) * len(PRE_FORMS)
    T.report(f"bnpre {name} (M {side.n}, N {bd.c.N}, C {bd.c.K})")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def null(g: Gb):
    return Gb(g.t, g.lo, g.n, True)


def _with(D, **kw):
    D2 = copy.deepcopy(D)
    for k, v in kw.items():
        if k.startswith("seg_"):
            setattr(D2.segs[0], k[4:], v)
        else:
            setattr(D2, k, v)
    return D2


def test_bnb_refusals(X):
    """zsg_conv_igemm_bnb / zsg_conv_wino_bnb (and the *_tail forms): split-K, N % 4 != 0, an out_off that is no multiple of 4, bn_x
    not 16-byte aligned, merge_x, NULL partials — rc -1, the entry named, every byte of every buffer as it was"""
    L, ops = X
    T = Tally()
    for name, kern, v in (("d_m722", "ig", (64, 64, 0, 0, 1, 0)), ("d_w107", "wn", (32, 64, 1, 1, 0)), ("d_w107", "ig", (128, 64, 1, 0, 1, 0))):
        bd = B.data(name)
        side = Side(L, ops, bd)
        D = bd.D
        for tail in (False, True):
            form = TAIL_FORMS[0] if tail else BNB_FORMS[0]
            what = f"{name} {kern} {'tail ' if tail else ''}"
            assert bnb_launch(L, side, kern, v, form, tail, T, what + "accepted as it stands", plain_check=False) is not None
            vs = v[:4] + (2, 0) if kern == "ig" else v[:3] + (2, 0)
            assert bnb_launch(L, side, kern, vs, form, tail, T, what + "split-K", want=-1) is None
            for label, D2 in (("N % 4 != 0", _with(D, N=D.N - 2)), ("out_off % 4 != 0", _with(D, seg_out_off=2)), ("merge_x", _with(D, merge_x=1))):
                s2 = copy.copy(side)
                s2.D = D2
                s2.part_rows = lambda L_, k_, v_, s=side: s.part_rows(L_, k_, v_)
                assert bnb_launch(L, s2, kern, v, form, tail, T, what + label, want=-1) is None
            s3 = copy.copy(side)
            s3.bn_x = Gb(side.bn_x.t, side.bn_x.lo + 1, side.bn_x.n - 1)
            assert bnb_launch(L, s3, kern, v, form, tail, T, what + "bn_x 4 bytes off 16-byte alignment", want=-1) is None
            s4 = copy.copy(side)
            s4._memo = dict(side._memo)
            prow = side.part_rows(L, kern, v)
            s4._memo[("pb", prow)] = null(side._memo[("pb", prow)])
            assert bnb_launch(L, s4, kern, v, form, tail, T, what + "NULL partials", want=-1) is None
    T.report("bnb refusals")


def test_finalize_refusals(X):
    """the *_bnstat / *_bnb_tail entries: no hint, BM = 32, split-K, NULL tickets / coef / mean — refused with nothing written;
    zsg_conv_bn_tail_tickets says -1 where the descriptor is the reason"""
    L, ops = X
    T = Tally()
    for fname, dname, kern, v in (("f_m722", "d_pw722", "ig", (64, 64, 0, 0, 1, 0)), ("f_w107", "d_w107", "wn", (64, 64, 0, 1, 0))):
        fs, ds = Side(L, ops, B.data(fname)), Side(L, ops, B.data(dname))
        bad = [("no hint", None)]
        if kern == "ig":
            bad += [("BM = 32", (32, 64, 0, 0, 1, 0)), ("split-K", (64, 64, 0, 0, 2, 0))]
        else:
            bad += [("split-K", (64, 64, 0, 2, 0))]
        assert bnstat_launch(L, fs, kern, v, True, T, f"{fname} {kern} accepted as it stands") is not None
        assert bnb_launch(L, ds, kern, v, TAIL_FORMS[0], True, T, f"{dname} {kern} accepted as it stands", plain_check=False) is not None
        for label, vb in bad:
            assert int(L.lib.zsg_conv_bn_tail_tickets(C.byref(desc_of(L, fs.D, kern, vb)), int(kern == "wn"))) == -1, label
            assert bnstat_launch(L, fs, kern, vb, True, T, f"{fname} {kern} bnstat {label}", want=-1) is None
            assert bnb_launch(L, ds, kern, vb, TAIL_FORMS[0], True, T, f"{dname} {kern} bnb_tail {label}", want=-1) is None
        # NULL arguments
        for key in (("tk", -(-fs.N // v[1])), "mo"):
            s2 = copy.copy(fs)
            s2._memo = dict(fs._memo)
            s2._memo[key] = null(fs._memo[key])
            assert bnstat_launch(L, s2, kern, v, True, T, f"{fname} {kern} bnstat NULL {key}", want=-1) is None
        for key in (("tk", -(-ds.N // v[1])), "coef"):
            s2 = copy.copy(ds)
            s2._memo = dict(ds._memo)
            s2._memo[key] = null(ds._memo[key])
            assert bnb_launch(L, s2, kern, v, TAIL_FORMS[0], True, T, f"{dname} {kern} bnb_tail NULL {key}", want=-1) is None
    T.report("finalize refusals")


def test_bnpre_refusals(X):
    """zsg_conv_igemm_bnpre: C = 48, a 3x3 or strided descriptor, a non-dense source, wc0 != 0, the 64-deep-K bit, the 4-wave 128x128
    tile, the streaming kernel, a ReLU epilogue, an unaligned pre_* pointer"""
    L, ops = X
    T = Tally()
    bd = B.data("p_m65")
    side = Side(L, ops, bd)
    D = bd.D
    v = (64, 64, 0, 0, 1, 0)
    form = PRE_FORMS[0]
    assert pre_launch(L, side, v, form, T, "p_m65 accepted as it stands") is not None
    D3 = _with(D, wR=3, wS=3)
    D3.segs[0].ty, D3.segs[0].tx = R.Taps(3, 0, 1, -1, 1), R.Taps(3, 0, 1, -1, 1)
    for label, D2 in (("C = 48", _with(D, C=48)), ("3x3", D3), ("strided", _with(D, seg_sy=2, seg_sx=2)), ("non-dense source", _with(D, src_ld=D.C + 4)),
                      ("wc0 != 0", _with(D, wc0=32, wC=D.C + 32)), ("relu = 1", _with(D, relu=1))):
        assert pre_launch(L, side, v, form, T, f"p_m65 {label}", want=-1, D=D2, word="conv") is None
    for label, vb in (("the 64-deep-K bit", (64, 64, 0, 1, 1, 0)), ("the 4-wave 128x128 tile", (128, 128, 0, 0, 1, 0)), ("the streaming kernel", (32, 64, 0, 0, 1, 0)),
                      ("split-K", (64, 64, 0, 0, 2, 0)), ("stream-K", (64, 64, 0, 0, 1, 1))):
        assert pre_launch(L, side, vb, PRE_FORMS[1], T, f"p_m65 {label}", want=-1, word="conv") is None
    for k in ("pre_mean", "pre_invstd", "pre_gamma", "pre_beta", "pre_res", "pre_y"):
        def tweak(a, k=k):
            a[k] += 4
        assert pre_launch(L, side, v, form, T, f"p_m65 {k} 4 bytes off 16-byte alignment", want=-1, tweak=tweak, word="conv_igemm_bnpre") is None
    T.report("bnpre refusals")

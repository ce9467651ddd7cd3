"""Host reference of the exact-arithmetic tests of the BatchNorm-fused convolution entries (tests/test_cpu_conv_bn_exact.py,
tests/test_gpu_conv_bn_exact.py): zsg_conv_igemm_bnb / zsg_conv_wino_bnb (BatchNorm-backward sums in the data gradient's epilogue),
zsg_conv_igemm_bnstat / zsg_conv_wino_bnstat / *_bnb_tail (the in-kernel finalize of csrc/bn_tail.h) and zsg_conv_igemm_bnpre (the
BatchNorm-applying operand loader).  Built on tests/conv_exact_ref.py: its Desc / View model, conv_rows, the partial-row layouts, the
operand builder and the guard / poison / sentinel conventions.  Nothing of the product is imported; every formula is include/zsg.h's:

    bnb       out = dgrad [+ add_src];  g = relu-bit ? out : +0;  xhat = (bn_x - mean) * invstd   (bn_x, the bits: at the OUTPUT's offsets)
              relu bits as zsg_bn_apply writes them: byte i holds elements 4i .. 4i+3, bit e = element 4i+e > 0, bits 4-7 zero
              partials[tile][0][n] = sum g, partials[tile][1][n] = sum g * xhat; a tile = BM output rows of a segment (b, y, x order)
              or TB Winograd tiles (2x2 pixels; pixels beyond an odd edge do not exist); epi_flags bit 0: the stored output is g
    finalize  forward  m = S / n, var = max(SS / n - m * m, 0), mean = f32(m), invstd = f32(1 / sqrt(var + eps)),
                       rmean = (1 - mom) * rmean + mom * f32(m), rvar = (1 - mom) * rvar + mom * f32(n > 1 ? var * n / (n - 1) : var)
              backward coef[0] = f32(S / n), coef[1] = f32(SS / n), dbeta = (acc ? dbeta : 0) + f32(S), dgamma likewise with SS
              n = the output rows of ALL segments
    bnpre     pre_y = relu((x - pre_mean) * pre_invstd * pre_gamma + pre_beta + pre_residual), its relu bits (an exact 0 has bit 0:
              "element > 0"), and the 1x1 convolution of pre_y with its fused statistics

Data: integers, with invstd / pre_invstd / pre_gamma powers of two (mixed exponents, gamma of both signs), so every stored output,
every partial-row element and every column total is an integer or a half-integer far below 2^24: exact in fp32 in any summation
order and under any fma contraction.  `exactness` returns the bounds, tests/test_cpu_conv_bn_exact.py asserts them per case.  The
bounds are taken over ABSOLUTE values (sum |g| (|x| + |mean|) invstd), so they also hold for a kernel that forms sum g*x and
mean * sum g separately.  The finalize divides and takes a square root in fp64 on the device: mean / invstd / coef / running statistics
are compared within 1 fp32 ulp of the fp64 values below (|S| < 2^23: a lost or doubled element moves S by at least 1/2, the quotient
by far more than an ulp).

mutate= (negative controls; every one must change the result of every case that lists the edge in `covers`):
    drop_last_row    the last tile of every segment loses its last row          count_overhang   a Winograd tile counts the pixels beyond
    shift_bit        channel n takes the relu bit of channel n + 1                               an odd edge (bit 1, bn_x read as 0)
    ignore_add       g = dgrad * bit (add_src forgotten in the sums)            n_minus_1        the finalize divides by n - 1
    skip_last_group  the last 16-byte column group is never summed              seg0_rows        n = nseg * (rows of segment 0)"""
import copy
from dataclasses import dataclass

import torch

import conv_exact_ref as R

DT = R.DT
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # the fp32 argument as the device widens it
MOM = 0.25
MUTATIONS = ("drop_last_row", "count_overhang", "shift_bit", "ignore_add", "n_minus_1", "skip_last_group", "seg0_rows")


@dataclass
class BCase:
    """mode 'dg': the data gradient of a convolution with N input and K output channels; `sizes` are the dx maps
    (the BatchNorm's maps), the reduction runs over K = dy.ld.  mode 'fw' / 'pre': a forward convolution K -> N over `sizes`
    ('pre': 1x1 with the BatchNorm-applying loader).  M = output rows, N = the BatchNorm's channels = the GEMM's columns."""
    name: str
    mode: str
    B: int
    K: int
    N: int
    sizes: list
    k: int = 1
    s: int = 1
    p: int = 0
    d: int = 1
    amp: int = 3
    amp_w: int = 3
    covers: tuple = ()

    def desc(self):
        k, s, p, d = self.k, self.s, self.p, self.d
        osz = [(R.conv_out(h, k, s, p, d), R.conv_out(w, k, s, p, d)) for h, w in self.sizes]
        if self.mode == "dg":
            return R.dgrad_desc(R.make_view(self.B, self.K, osz), R.make_view(self.B, self.N, self.sizes), self.N, k, s, p, d)
        return R.fwd_desc(R.make_view(self.B, self.K, self.sizes), R.make_view(self.B, self.N, osz), self.K, self.N, k, s, p, d, self.K)

    @property
    def wino(self):
        return self.mode != "pre" and (self.k, self.s, self.p, self.d) == (3, 1, 1, 1)


PYR = R.PYR
# covers: the mutations (module docstring) the case's data must tell from the truth
_DG = ("shift_bit", "ignore_add", "drop_last_row", "skip_last_group", "n_minus_1")
CASES = [
    # ---- data gradients (bnb, bnb_tail)
    BCase("d_m1", "dg", 1, 64, 64, [(1, 1)], covers=_DG),                                               # M = 1: one row tile, rows == 1
    BCase("d_m65", "dg", 1, 36, 68, [(5, 13)], covers=_DG),                                             # M = 65, N = 68, K = 36
    BCase("d_m722", "dg", 2, 40, 96, [(19, 19)], covers=_DG),                                           # M = 722, N = 96, K = 40
    BCase("d_n132", "dg", 1, 64, 132, [(5, 13)], 3, 1, 1, covers=_DG + ("count_overhang",)),            # N = 132; 3x3; wino BN = 32: 4 + 4 channels
    BCase("d_s2", "dg", 1, 64, 64, [(21, 21)], 3, 2, 1, covers=_DG + ("seg0_rows",)),                    # four parity segments
    BCase("d_dil6", "dg", 1, 64, 64, [(12, 12)], 3, 1, 6, 6, covers=_DG),
    BCase("d_w1", "dg", 1, 32, 36, [(1, 1)], 3, 1, 1, covers=_DG + ("count_overhang",)),                # Winograd maps 1x1 .. 19x19
    BCase("d_w3", "dg", 2, 64, 64, [(3, 3)], 3, 1, 1, covers=_DG + ("count_overhang",)),
    BCase("d_w5", "dg", 1, 36, 36, [(5, 5)], 3, 1, 1, covers=_DG + ("count_overhang",)),
    BCase("d_w107", "dg", 2, 40, 96, [(10, 7)], 3, 1, 1, covers=_DG + ("count_overhang",)),
    BCase("d_w19", "dg", 2, 64, 64, [(19, 19)], 3, 1, 1, amp=2, amp_w=2, covers=_DG + ("count_overhang",)),
    BCase("d_pyr", "dg", 2, 64, 64, PYR, 3, 1, 1, covers=_DG + ("seg0_rows", "count_overhang")),
    BCase("d_sk1024", "dg", 1, 1024, 64, [(5, 13)], amp=1, amp_w=1, covers=_DG),                        # stream-K: 2 tiles, K = 1024
    BCase("d_sk32", "dg", 2, 32, 64, [(19, 19)], covers=_DG),                                           # stream-K: K = 32 (one K step)
    BCase("d_r128", "dg", 2, 32, 64, [(64, 64)], amp=1, amp_w=1, covers=("n_minus_1",)),                # 128 rows at BM 64 / 64 at BM 128
    BCase("d_r129", "dg", 1, 32, 64, [(86, 96)], amp=1, amp_w=1),                                        # 129 rows at BM 64
    BCase("d_r128b", "dg", 1, 32, 64, [(128, 128)], amp=1, amp_w=1, covers=("n_minus_1",)),             # 128 rows at BM 128
    BCase("d_r129b", "dg", 1, 32, 64, [(129, 128)], amp=1, amp_w=1),                                     # 129 rows at BM 128
    BCase("d_pw1", "dg", 1, 64, 128, [(1, 1)], covers=_DG),                                             # the streaming 1x1 kernel: M = 1, 33, 722
    BCase("d_pw33", "dg", 1, 512, 128, [(3, 11)], amp=1, covers=_DG),                                   # (K = 512: only 32-wide units fit the LDS)
    BCase("d_pw33n", "dg", 1, 128, 512, [(3, 11)], covers=_DG),                                         # ... cut into four filter panels
    BCase("d_pw722", "dg", 2, 64, 128, [(19, 19)], covers=_DG),
    BCase("d_pw722k", "dg", 2, 512, 128, [(19, 19)], amp=1, amp_w=1, covers=_DG),
    # ---- forwards (bnstat)
    BCase("f_m1", "fw", 1, 64, 64, [(1, 1)], covers=("n_minus_1",)),
    BCase("f_m65", "fw", 1, 36, 68, [(5, 13)], covers=("n_minus_1", "drop_last_row", "skip_last_group")),
    BCase("f_m722", "fw", 2, 40, 96, [(19, 19)], amp=2, covers=("n_minus_1", "drop_last_row", "skip_last_group")),
    BCase("f_n132", "fw", 1, 64, 132, [(5, 13)], 3, 1, 1, amp=2, amp_w=2, covers=("n_minus_1", "drop_last_row", "count_overhang")),
    BCase("f_dil6", "fw", 1, 64, 64, [(12, 12)], 3, 1, 6, 6, amp=2, amp_w=2, covers=("n_minus_1",)),
    BCase("f_w1", "fw", 1, 32, 36, [(1, 1)], 3, 1, 1, covers=("n_minus_1", "count_overhang")),
    BCase("f_w5", "fw", 1, 36, 36, [(5, 5)], 3, 1, 1, covers=("n_minus_1", "count_overhang")),
    BCase("f_w107", "fw", 2, 40, 96, [(10, 7)], 3, 1, 1, amp=2, amp_w=2, covers=("n_minus_1", "count_overhang")),
    BCase("f_w19", "fw", 2, 64, 64, [(19, 19)], 3, 1, 1, amp=1, amp_w=2, covers=("n_minus_1", "count_overhang")),
    BCase("f_pyr", "fw", 2, 64, 64, PYR, 3, 1, 1, amp=2, amp_w=2, covers=("n_minus_1", "seg0_rows", "count_overhang")),
    BCase("f_sk1024", "fw", 1, 1024, 64, [(5, 13)], amp=1, amp_w=1, covers=("n_minus_1",)),
    BCase("f_sk32", "fw", 2, 32, 64, [(19, 19)], covers=("n_minus_1",)),
    BCase("f_r128", "fw", 2, 32, 64, [(64, 64)], amp=1, amp_w=1, covers=("n_minus_1",)),
    BCase("f_r129", "fw", 1, 32, 64, [(86, 96)], amp=1, amp_w=1),
    BCase("f_r128b", "fw", 1, 32, 64, [(128, 128)], amp=1, amp_w=1, covers=("n_minus_1",)),
    BCase("f_r129b", "fw", 1, 32, 64, [(129, 128)], amp=1, amp_w=1),
    # ---- the BatchNorm-applying loader (bnpre): C = 32, 96, 256; M = 1, 65, 722; N = 64, 68, 132
    BCase("p_m1", "pre", 1, 32, 64, [(1, 1)], covers=("n_minus_1",)),
    BCase("p_m65", "pre", 1, 96, 68, [(5, 13)], amp_w=1, covers=("n_minus_1", "drop_last_row", "skip_last_group")),
    BCase("p_m722", "pre", 2, 32, 132, [(19, 19)], amp_w=1, covers=("n_minus_1", "drop_last_row", "skip_last_group")),
    BCase("p_c256", "pre", 1, 256, 64, [(10, 7)], amp_w=1, covers=("n_minus_1", "drop_last_row")),
]
CASE = {c.name: c for c in CASES}


def f32(v):
    """round a float64 tensor to fp32 and widen it again"""
    return v.float().double()


def pack_bits(bits):
    """zsg_bn_apply's layout: byte i = elements 4i .. 4i+3, bit e = element 4i+e (include/zsg.h)"""
    b = bits.reshape(-1, 4).to(torch.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


def partial_rows(pairs, BM, mutate=None):
    """[tiles][2][N] of per-row quantities (a, b) per segment: tile t of a segment sums its rows t*BM .. t*BM+BM-1 ((b, y, x) order)"""
    rows = []
    for a, b in pairs:
        fa, fb = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
        for r0 in range(0, fa.shape[0], BM):
            ta, tb = fa[r0:r0 + BM], fb[r0:r0 + BM]
            if mutate == "drop_last_row" and r0 + BM >= fa.shape[0]:
                ta, tb = ta[:-1], tb[:-1]
            rows.append(torch.stack([ta.sum(0), tb.sum(0)]))
    return torch.stack(rows)


def wino_partial_rows(pairs, TB, over=None, mutate=None):
    """a row per TB Winograd tiles (2x2 output pixels, tile index (b * ceil(H/2) + ty) * ceil(W/2) + tx) per segment; `over`: per segment
    the (a, b) a tile would hold at pixels beyond an odd edge ([B, He, We, N], the count_overhang mutation)"""
    rows = []
    for si, (a, b) in enumerate(pairs):
        B, H, W, N = a.shape
        He, We = (H + 1) // 2 * 2, (W + 1) // 2 * 2
        s = []
        for j, v in enumerate((a, b)):
            pad = torch.zeros(B, He, We, N, dtype=DT) if over is None else over[si][j].clone()
            pad[:, :H, :W] = v
            s.append(pad.view(B, He // 2, 2, We // 2, 2, N).sum((2, 4)).reshape(-1, N))
        nt = s[0].shape[0]
        for r0 in range(0, nt, TB):
            sa, sb = s[0][r0:r0 + TB], s[1][r0:r0 + TB]
            if mutate == "drop_last_row" and r0 + TB >= nt:          # (the last Winograd tile of the segment's last row tile)
                sa, sb = sa[:-1], sb[:-1]
            rows.append(torch.stack([sa.sum(0), sb.sum(0)]))
    return torch.stack(rows)


def total_rows(D):
    return sum(D.B * g.rows_y * g.rows_x for g in D.segs)


def finalize_n(D, mutate=None):
    n = total_rows(D)
    if mutate == "seg0_rows":
        n = D.nseg * D.B * D.segs[0].rows_y * D.segs[0].rows_x
    if mutate == "n_minus_1":
        n -= 1
    return float(n)


def finalize_fwd(S, SS, n, rm0=None, rv0=None, eps=EPS, mom=MOM):
    """fp64 values whose fp32 roundings the device publishes: mean, invstd, running_mean, running_var"""
    m = S / n
    var = torch.clamp(SS / n - m * m, min=0)
    unb = var * n / (n - 1) if n > 1 else var
    return {"mean": m, "invstd": 1.0 / torch.sqrt(var + eps),
            "rmean": None if rm0 is None else (1 - mom) * rm0 + mom * f32(m),
            "rvar": None if rv0 is None else (1 - mom) * rv0 + mom * f32(unb)}


def finalize_bwd(S, SS, n, acc, dg0, db0):
    return {"coef": torch.stack([S / n, SS / n]), "dbeta": (db0 if acc else 0) + f32(S), "dgamma": (dg0 if acc else 0) + f32(SS)}


class BData:
    """operands and references of one case (computed once, shared, never modified)"""

    def __init__(self, c: BCase):
        self.c = c
        g = torch.Generator().manual_seed(4000 + sum(map(ord, c.name)))
        self.D = D = c.desc()
        N = c.N
        self.x_idx, self.w_idx, self.o_idx = R.src_addressed(D), R.wt_index(D), R.out_written(D)
        self.ext = R.out_extent(D)
        assert len(self.o_idx) == self.ext == total_rows(D) * N and len(torch.unique(self.o_idx)) == self.ext, "dense, fully covered output"
        assert self.w_idx.numel() == R.wt_extent(D)
        self.w = R.rand_int((R.wt_extent(D),), c.amp_w, g)
        # multiples of 4: (1 - 1/4) * r is exact; large against any mean / 4, so that the update never cancels (an ulp of f32(m) stays
        # below an ulp of the result)
        self.rm0 = 4.0 * torch.randint(64, 129, (N,), generator=g).to(DT)
        self.rv0 = 4.0 * torch.randint(1, 5, (N,), generator=g).to(DT)
        self._memo = {}
        if c.mode == "pre":
            self._pre(g)
            return
        self.x = torch.full((R.src_extent(D),), R.POISON, dtype=DT)
        self.x[self.x_idx] = R.rand_int((len(self.x_idx),), c.amp, g)
        self.rows = R.conv_rows(D, self.x, self.w)
        if c.mode != "dg":
            return
        self.add = R.rand_int((self.ext,), 3, g)
        self.bn_x = R.rand_int((self.ext,), 3, g)
        self.mean = torch.randint(-2, 3, (N,), generator=g).to(DT)
        self.invstd = 2.0 ** torch.randint(-1, 3, (N,), generator=g).to(DT)               # 1/2, 1, 2, 4
        bits = torch.randint(0, 2, (self.ext // N, N), generator=g)
        # zeros and ones in every row (hence every tail row and every Winograd overhang neighbour) and in every row's last column group
        bits[:, 0], bits[:, 1] = 0, 1
        bits[0::2, N - 4:] = torch.tensor([1, 0, 0, 1])
        bits[1::2, N - 4:] = torch.tensor([0, 1, 1, 0])
        self.bits = bits.reshape(-1).to(DT)
        self.dg0, self.db0 = R.rand_int((N,), 5, g), R.rand_int((N,), 5, g)

    # ---- bnpre ------------------------------------------------------------------------------------------------------------------------
    def _pre(self, g):
        c, D = self.c, self.D
        M, Cc = total_rows(D), c.K
        assert len(self.x_idx) == M * Cc == R.src_extent(D), "dense source"
        self.x = 4.0 * R.rand_int((M, Cc), 3, g)                                          # multiples of 4: (x - mean) * scale is an integer
        self.pre_mean = 4.0 * torch.randint(-1, 2, (Cc,), generator=g).to(DT)
        self.pre_invstd = 2.0 ** torch.randint(-1, 1, (Cc,), generator=g).to(DT)          # 1/2, 1
        self.pre_gamma = 2.0 ** torch.randint(-1, 2, (Cc,), generator=g).to(DT) * (torch.randint(0, 2, (Cc,), generator=g).to(DT) * 2 - 1)
        self.pre_beta = R.rand_int((Cc,), 3, g)
        base = (self.x - self.pre_mean) * self.pre_invstd * self.pre_gamma + self.pre_beta
        assert torch.equal(base, base.round())
        res = R.rand_int((M, Cc), 6, g)
        zero = torch.rand((M, Cc), generator=g) < 0.125                                   # exact zeros before the ReLU: bit 0
        res = torch.where(zero, -base, res)
        tgt = torch.tensor([2.0, 0.0, -3.0, 1.0], dtype=DT)                               # every row's last column group: +, 0, -, +
        res[:, Cc - 4:] = tgt - base[:, Cc - 4:]
        res[:, 0] = 1.0 - base[:, 0]
        self.pre_res = res
        v = base + res
        self.pre_v = v
        self.pre_y = torch.clamp(v, min=0)
        self.pre_bits = (v > 0).to(DT)
        self.rows = R.conv_rows(D, self.pre_y.reshape(-1), self.w)

    # ---- bnb --------------------------------------------------------------------------------------------------------------------------
    def _over(self, mask):
        """what a Winograd tile would hold at the pixels beyond an odd edge: the convolution continued there, bit 1, bn_x read as 0"""
        D2 = copy.deepcopy(self.D)
        for s in D2.segs:
            s.rows_y, s.rows_x = (s.rows_y + 1) // 2 * 2, (s.rows_x + 1) // 2 * 2
        out = []
        for acc in R.conv_rows(D2, self.x, self.w):
            if self.c.mode == "dg":
                out.append((acc, acc * ((0 - self.mean) * self.invstd)))
            else:
                out.append((acc, acc * acc))
        return out

    def bnb(self, tile, wino=False, mask=True, add=True, epi=0, mutate=None):
        """-> (flat stored output, partial rows [tiles][2][N]); tile = BM (or TB, wino); tile None: one row over everything (the
        streaming kernel's column totals)"""
        key = ("bnb", tile, wino, mask, add, epi, mutate)
        if key in self._memo:
            return self._memo[key]
        D, N = self.D, self.c.N
        out = torch.zeros(self.ext, dtype=DT)
        pairs = []
        for si, acc in enumerate(self.rows):
            oi = R.out_index(D, si)
            v = acc + self.add[oi] if add else acc
            bit = self.bits[oi] if mask else torch.ones_like(acc)
            if mutate == "shift_bit":
                bit = torch.roll(bit, -1, -1)
            zero = torch.zeros_like(acc)          # (a cleared element is +0 whatever the sign of the sum: a select, not a product)
            gr = torch.where(bit > 0, acc if mutate == "ignore_add" else v, zero)
            xh = (self.bn_x[oi] - self.mean) * self.invstd
            out[oi] = torch.where(bit > 0, v, zero) if epi else v
            pairs.append((gr, gr * xh))
        part = self._part(pairs, tile, wino, mutate)
        self._memo[key] = (out, part)
        return out, part

    def _part(self, pairs, tile, wino, mutate):
        if tile is None:
            part = partial_rows(pairs, 1 << 30, mutate).sum(0, keepdim=True)
        elif wino:
            part = wino_partial_rows(pairs, tile, self._over(True) if mutate == "count_overhang" else None, mutate)
        else:
            part = partial_rows(pairs, tile, mutate)
        if mutate == "skip_last_group":
            part = part.clone()
            part[:, :, self.c.N - 4:] = 0
        return part

    def stat(self, tile, wino=False, mutate=None):
        """forward statistics: partial rows (sum, sum of squares) of the convolution output"""
        key = ("stat", tile, wino, mutate)
        if key not in self._memo:
            self._memo[key] = self._part([(a, a * a) for a in self.rows], tile, wino, mutate)
        return self._memo[key]

    def out_flat(self):
        out = torch.zeros(self.ext, dtype=DT)
        for si, acc in enumerate(self.rows):
            out[R.out_index(self.D, si)] = acc
        return out


_DATA = {}


def data(name) -> BData:
    if name not in _DATA:
        _DATA[name] = BData(CASE[name])
    return _DATA[name]


def exactness(bd: BData):
    """the fp32 bounds of a case from the reference alone (all over absolute values: order-independent)"""
    c, D = bd.c, bd.D
    src = bd.pre_y.reshape(-1) if c.mode == "pre" else bd.x
    conv_abs = max(float(r.max()) for r in R.conv_rows(D, src.abs(), bd.w.abs()))
    rows = torch.cat([r.reshape(-1, c.N) for r in bd.rows])
    e = {"conv_abs": conv_abs, "S_abs": float(rows.abs().sum(0).max()), "SS": float((rows * rows).sum(0).max())}
    if c.mode == "dg":
        out = (bd.out_flat().abs() + bd.add.abs()).view(-1, c.N)
        xh = (bd.bn_x.abs().view(-1, c.N) + bd.mean.abs()) * bd.invstd
        e["S_abs"] = float(out.sum(0).max())
        e["SS"] = 2 * float((out * xh).sum(0).max())          # (half-integers: one bit more)
        e["acc_abs"] = max(float(bd.dg0.abs().max()), float(bd.db0.abs().max()))
    if c.mode == "pre":
        e["pre_abs"] = float(((bd.x.abs() + bd.pre_mean.abs()) * bd.pre_invstd * bd.pre_gamma.abs() + bd.pre_beta.abs() + bd.pre_res.abs()).max()) * 4
    return e

"""Host reference and operand builder of the exact-arithmetic fp32 convolution tests (tests/test_cpu_conv_exact.py,
tests/test_gpu_conv_exact.py).  Nothing of the product is imported: the descriptor below is a plain-Python copy of zsg_conv_desc /
zsg_seg / zsg_taps (include/zsg.h) and every routine is written tap by tap from that header's definition:

    a segment enumerates output rows (b, y, x) over rows_y x rows_x per image; row (b, y, x) and tap (jy, jx) gather the source pixel
        (y*sy + ty.d0 + jy*ty.dstep,  x*sx + tx.d0 + jx*tx.dstep)          (zero outside [0, src_H) x [0, src_W))
    and multiply it with weight tap (ty.w0 + jy*ty.wstep, tx.w0 + jx*tx.wstep); weight row n starts at n*wt_ld, tap (r, s) at
    (r*wS + s)*wC, the channels used are wc0 .. wc0+C-1; the row is stored at output pixel (y*osy + opy, x*osx + opx) of an out_W-wide
    image.  out = epilogue(sum): + bias[n]; + add_src[same index as out]; relu; * (mask_src[same index] > 0).

All data are small non-zero integers held in float64 (exact: every sum stays far below 2^53), so the results are THE integers the
fp32 kernels must produce bit for bit whatever their summation order — as long as the fp32 bounds of `exactness` hold, which
tests/test_cpu_conv_exact.py asserts from this reference alone.

Operand builder (Buf): every operand lies in one flat buffer with GUARD NaN elements in front and behind.  Inside an operand's extent
every element the descriptor does NOT address (row padding C..src_ld-1, gaps between images and levels, weight channels outside
[wc0, wc0+C), wt_ld slack) holds the finite poison 2^20: exact, harmless against a zero partner, fatal to equality against anything
else.  ONE exception, where the contract makes padding part of the operand: a data-gradient descriptor reduces over C_red = dy.ld
channels, so dy's pad lanes N..ld-1 and the weight image's pad columns are operand elements and hold the zeros the contract requires
(dgrad_desc below; zsg_transpose_w writes those zeros).  Outputs are pre-filled with NaN where the launch must write; everything else
of an output buffer — both guards, pad lanes N..out_ld-1, gaps, weight-gradient channels outside the window, rows of other levels —
holds SENTINEL and must come back unchanged."""
from dataclasses import dataclass, field
from typing import List, Optional

import torch

GUARD = 4096
POISON = float(2 ** 20)
SENTINEL = -1234567.0           # exact in fp32; no case can produce it (every written value is a small integer)
DT = torch.float64


# ---- descriptor (include/zsg.h) -----------------------------------------------------------------------------------------------------
@dataclass
class Taps:
    n: int
    w0: int
    wstep: int
    d0: int
    dstep: int


@dataclass
class Seg:
    rows_y: int
    rows_x: int
    src_H: int
    src_W: int
    sy: int
    sx: int
    out_W: int
    osy: int
    osx: int
    opy: int
    opx: int
    src_off: int
    src_bstride: int
    out_off: int
    out_bstride: int
    ty: Taps
    tx: Taps


@dataclass
class Desc:
    B: int
    C: int
    N: int
    src_ld: int
    out_ld: int
    wR: int
    wS: int
    wC: int
    wc0: int
    wt_ld: int
    relu: int = 0
    merge_x: int = 0
    segs: List[Seg] = field(default_factory=list)
    zero_fill: bool = False          # data gradient only: parity classes without any tap are not launched, the caller clears dx

    @property
    def nseg(self):
        return len(self.segs)


@dataclass
class Lvl:
    off: int
    H: int
    W: int
    bstride: int


@dataclass
class View:
    """an NHWC activation (or a pyramid sharing one buffer): element (l, b, y, x, c) at levels[l].off + b*bstride + (y*W + x)*ld + c"""
    B: int
    C: int
    ld: int
    levels: List[Lvl]

    def extent(self):
        return max(l.off + (self.B - 1) * l.bstride + l.H * l.W * self.ld for l in self.levels)

    def index(self, li, C=None):
        """[B, H, W, C] flat element indices of level li"""
        l = self.levels[li]
        b = torch.arange(self.B).view(-1, 1, 1, 1)
        y = torch.arange(l.H).view(1, -1, 1, 1)
        x = torch.arange(l.W).view(1, 1, -1, 1)
        c = torch.arange(self.C if C is None else C).view(1, 1, 1, -1)
        return l.off + b * l.bstride + (y * l.W + x) * self.ld + c


def conv_out(n, k, s, p, d=1):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def make_view(B, C, sizes, ld=None, off=0, gap=0, scatter=False):
    """levels one behind the other (images H*W*ld + gap apart, `gap` more between levels), or `scatter`: the [B, P, ld] layout of the
    shared head's outputs (level l starts P_l pixels into every image's row block)"""
    ld = ld or C
    lv = []
    if scatter:
        P = sum(h * w for h, w in sizes)
        px = 0
        for h, w in sizes:
            lv.append(Lvl(off + px * ld, h, w, P * ld + gap))
            px += h * w
    else:
        o = off
        for h, w in sizes:
            bs = h * w * ld + gap
            lv.append(Lvl(o, h, w, bs))
            o += B * bs + gap
    return View(B, C, ld, lv)


def fwd_desc(src: View, out: View, C, N, k, s, p, d, wC, wc0=0, wt_ld=None, relu=False, merge_x=False):
    """forward convolution; with `out` = the dy view it is also the weight gradient's descriptor"""
    D = Desc(src.B, C, N, src.ld, out.ld, k, k, wC, wc0, wt_ld if wt_ld is not None else k * k * wC, int(relu), int(merge_x))
    for ls, lo in zip(src.levels, out.levels):
        assert lo.H == conv_out(ls.H, k, s, p, d) and lo.W == conv_out(ls.W, k, s, p, d)
        D.segs.append(Seg(lo.H, lo.W, ls.H, ls.W, s, s, lo.W, 1, 1, 0, 0, ls.off, ls.bstride, lo.off, lo.bstride,
                          Taps(k, 0, 1, -p, d), Taps(k, 0, 1, -p, d)))
    return D


def dgrad_desc(dy: View, dx: View, N, k, s, p, d):
    """data gradient over the transposed weight image WT[cin][k][k][C_red], C_red = dy.ld (pad lanes are operand zeros, see the module
    docstring).  dx pixel Y = y*s + py receives dy pixel q through tap r iff Y = q*s - p + r*d.  Stride 1: q = Y + p - r*d for every r.
    Stride s (d = 1): r = r0 + j*s with r0 = (py + p) mod s, q = y + (py + p - r0)/s - j: one segment per parity class (py, px); a class
    without taps writes nothing (zero_fill)."""
    C = dy.ld
    D = Desc(dy.B, C, N, dy.ld, dx.ld, k, k, C, 0, k * k * C)
    for ly, lx in zip(dy.levels, dx.levels):
        assert ly.H == conv_out(lx.H, k, s, p, d) and ly.W == conv_out(lx.W, k, s, p, d)
        if s == 1:
            D.segs.append(Seg(lx.H, lx.W, ly.H, ly.W, 1, 1, lx.W, 1, 1, 0, 0, ly.off, ly.bstride, lx.off, lx.bstride,
                              Taps(k, 0, 1, p, -d), Taps(k, 0, 1, p, -d)))
            continue
        assert d == 1
        for py in range(s):
            ry = len(range(py, lx.H, s))
            r0 = (py + p) % s
            ty = Taps(len(range(r0, k, s)), r0, s, (py + p - r0) // s, -1)
            for px in range(s):
                rx = len(range(px, lx.W, s))
                c0 = (px + p) % s
                tx = Taps(len(range(c0, k, s)), c0, s, (px + p - c0) // s, -1)
                if ry <= 0 or rx <= 0:
                    continue
                if ty.n == 0 or tx.n == 0:
                    D.zero_fill = True
                    continue
                D.segs.append(Seg(ry, rx, ly.H, ly.W, 1, 1, lx.W, s, s, py, px, ly.off, ly.bstride, lx.off, lx.bstride, ty, tx))
    return D


# ---- index sets -----------------------------------------------------------------------------------------------------------------------
def out_index(D: Desc, si, N=None):
    """[B, rows_y, rows_x, N] flat indices of segment si's output rows"""
    g = D.segs[si]
    b = torch.arange(D.B).view(-1, 1, 1, 1)
    y = torch.arange(g.rows_y).view(1, -1, 1, 1)
    x = torch.arange(g.rows_x).view(1, 1, -1, 1)
    n = torch.arange(D.N if N is None else N).view(1, 1, 1, -1)
    return g.out_off + b * g.out_bstride + ((y * g.osy + g.opy) * g.out_W + (x * g.osx + g.opx)) * D.out_ld + n


def out_written(D: Desc):
    return torch.cat([out_index(D, i).reshape(-1) for i in range(D.nseg)])


def src_addressed(D: Desc):
    """the source operand: channels 0..C-1 of every pixel of every segment's image"""
    idx = []
    for g in D.segs:
        b = torch.arange(D.B).view(-1, 1, 1)
        px = torch.arange(g.src_H * g.src_W).view(1, -1, 1)
        c = torch.arange(D.C).view(1, 1, -1)
        idx.append((g.src_off + b * g.src_bstride + px * D.src_ld + c).reshape(-1))
    return torch.unique(torch.cat(idx))


def src_extent(D: Desc):
    return max(g.src_off + (D.B - 1) * g.src_bstride + g.src_H * g.src_W * D.src_ld for g in D.segs)


def out_extent(D: Desc):
    return max(g.out_off + (D.B - 1) * g.out_bstride + ((g.rows_y - 1) * g.osy + g.opy + 1) * g.out_W * D.out_ld for g in D.segs)


def wt_index(D: Desc):
    """[N, wR, wS, C] flat indices of the weight window"""
    n = torch.arange(D.N).view(-1, 1, 1, 1)
    r = torch.arange(D.wR).view(1, -1, 1, 1)
    s = torch.arange(D.wS).view(1, 1, -1, 1)
    c = torch.arange(D.C).view(1, 1, 1, -1)
    return n * D.wt_ld + (r * D.wS + s) * D.wC + D.wc0 + c


def wt_extent(D: Desc):
    return D.N * D.wt_ld


# ---- the convolution, tap by tap ------------------------------------------------------------------------------------------------------
def _tap_iter(D: Desc, g: Seg, mutate=None):
    """(jy, jx, valid y rows, source y, valid x rows, source x, weight tap r, s) of one segment"""
    y, x = torch.arange(g.rows_y), torch.arange(g.rows_x)
    for jy in range(g.ty.n):
        yy = y * g.sy + g.ty.d0 + jy * g.ty.dstep
        for jx in range(g.tx.n):
            xx = x * g.sx + g.tx.d0 + jx * g.tx.dstep
            if mutate == "shift_tap" and jy == 0 and jx == 0:
                xx = xx + 1                                   # negative control: the first tap reads its right-hand neighbour
            oy, ox = (yy >= 0) & (yy < g.src_H), (xx >= 0) & (xx < g.src_W)
            yield jy, jx, oy.nonzero().view(-1), yy[oy], ox.nonzero().view(-1), xx[ox], g.ty.w0 + jy * g.ty.wstep, g.tx.w0 + jx * g.tx.wstep


def _gather(D: Desc, g: Seg, src, ys, xs, ch):
    b = torch.arange(D.B).view(-1, 1, 1, 1)
    pix = ((ys.view(-1, 1) * g.src_W + xs.view(1, -1)) * D.src_ld).view(1, len(ys), len(xs), 1)
    return src[g.src_off + b * g.src_bstride + pix + ch.view(1, 1, 1, -1)]


def _channels(D: Desc, g: Seg, jy, jx, mutate, klast):
    """the reduction channels of a tap; 'drop_last_k': the last tap loses channel klast (default C-1: the last K element)"""
    ch = torch.arange(D.C)
    if mutate == "drop_last_k" and jy == g.ty.n - 1 and jx == g.tx.n - 1:
        ch = ch[ch != (D.C - 1 if klast is None else klast)]
    return ch


def conv_rows(D: Desc, src, wt, mutate=None, klast=None):
    """src, wt: flat float64 operands (element i of the operand at index i, no guards) -> per segment acc[B, rows_y, rows_x, N].
    mutate (negative controls of the tests): 'drop_last_k' omits the last channel of the last tap (klast: the last channel that is
    not an operand zero of a data gradient's padded dy rows), 'shift_tap' moves the first tap one pixel, 'drop_seg' omits the last segment (a parity class / a pyramid level)."""
    accs = []
    wi = wt_index(D)
    for si, g in enumerate(D.segs):
        acc = torch.zeros(D.B, g.rows_y, g.rows_x, D.N, dtype=DT)
        if mutate == "drop_seg" and si == D.nseg - 1:
            accs.append(acc)
            continue
        for jy, jx, iy, ys, ix, xs, r, s in _tap_iter(D, g, mutate):
            if len(iy) == 0 or len(ix) == 0:
                continue
            ch = _channels(D, g, jy, jx, mutate, klast)
            A = _gather(D, g, src, ys, xs, ch)                                   # [B, ny, nx, nc]
            W = wt[wi[:, r, s][:, ch]]                                           # [N, nc]
            acc[:, iy.view(-1, 1), ix.view(1, -1)] += A @ W.t()
        accs.append(acc)
    return accs


def epilogue(acc, bias=None, add=None, relu=False, mask=None):
    """include/zsg.h: + bias[n]; + add_src; relu; * (mask_src > 0)   (add / mask: gathered at the output's indices)"""
    v = acc.clone()
    if bias is not None:
        v = v + bias
    if add is not None:
        v = v + add
    if relu:
        v = torch.clamp(v, min=0)
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    return v


def forward(D: Desc, src, wt, out_init, bias=None, add=None, mask=None, mutate=None):
    """the whole launch on flat operands: returns the flat output (out_init where nothing is written); add / mask are flat buffers
    indexed like the output (add may be out_init itself: accumulate)"""
    out = out_init.clone()
    for si, acc in enumerate(conv_rows(D, src, wt, mutate)):
        if mutate == "drop_seg" and si == D.nseg - 1:
            continue
        oi = out_index(D, si)
        out[oi] = epilogue(acc, bias, None if add is None else add[oi], D.relu, None if mask is None else mask[oi])
    return out


def wgrad(D: Desc, src, dy, dw_init, accumulate, mutate=None):
    """dw[n][(r*wS+s)*wC + wc0 + c] (+)= sum_rows dy[row][n] * src[gather(row, r, s)][c]; D is the forward descriptor ("out" = dy);
    the segments (pyramid levels) add.  Elements outside the window keep dw_init."""
    wi = wt_index(D)
    acc = torch.zeros(D.N, D.wR, D.wS, D.C, dtype=DT)
    for si, g in enumerate(D.segs):
        if mutate == "drop_seg" and si == D.nseg - 1:
            continue
        G = dy[out_index(D, si)]                                                 # [B, ry, rx, N]
        for jy, jx, iy, ys, ix, xs, r, s in _tap_iter(D, g, mutate):
            if len(iy) == 0 or len(ix) == 0:
                continue
            ch = _channels(D, g, jy, jx, mutate, None)
            A = _gather(D, g, src, ys, xs, ch).reshape(-1, len(ch))
            Gt = G[:, iy.view(-1, 1), ix.view(1, -1)].reshape(-1, D.N)
            acc[:, r, s, :len(ch)] += Gt.t() @ A
    dw = dw_init.clone()
    dw[wi] = acc + (dw_init[wi] if accumulate else 0)
    return dw


def tile_partials(accs, BM):
    """bn_partials of zsg_conv_igemm: [m_tiles][2][N], m_tiles = sum over segments of ceil(rows / BM); tile t of a segment holds the
    column (sum, sum of squares) of its rows t*BM .. t*BM+BM-1 in (b, y, x) order"""
    rows = []
    for acc in accs:
        f = acc.reshape(-1, acc.shape[-1])
        for r0 in range(0, f.shape[0], BM):
            t = f[r0:r0 + BM]
            rows.append(torch.stack([t.sum(0), (t * t).sum(0)]))
    return torch.stack(rows)


def wino_tile_partials(accs, TB):
    """bn_partials of zsg_conv_wino: a row per TB Winograd tiles (2x2 output pixels, tile index (b*ceil(H/2) + ty)*ceil(W/2) + tx) per
    segment; pixels beyond an odd image edge do not exist"""
    rows = []
    for acc in accs:
        B, H, W, N = acc.shape
        pad = torch.zeros(B, (H + 1) // 2 * 2, (W + 1) // 2 * 2, N, dtype=DT)
        pad[:, :H, :W] = acc
        t = pad.view(B, (H + 1) // 2, 2, (W + 1) // 2, 2, N)
        s1, s2 = t.sum((2, 4)).reshape(-1, N), (t * t).sum((2, 4)).reshape(-1, N)
        for r0 in range(0, s1.shape[0], TB):
            rows.append(torch.stack([s1[r0:r0 + TB].sum(0), s2[r0:r0 + TB].sum(0)]))
    return torch.stack(rows)


# ---- Winograd --------------------------------------------------------------------------------------------------------------------------
WINO_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=DT)            # F(2x2,3x3) filter transform
WINO_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=DT)   # input transform
WINO_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=DT)                                # output transform
# F(3x3,2x2), the weight gradient: dy tiles take the place of the filter (2 taps), 3x3 outputs per 4x4 input tile
WINOWG_G = torch.tensor([[1, 0], [.5, .5], [.5, -.5], [0, 1]], dtype=DT)
WINOWG_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]], dtype=DT)
WINOWG_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], dtype=DT)


def wino_amplification(G=WINO_G, BT=WINO_BT, AT=WINO_AT):
    """Bound of the largest Winograd-domain partial sum relative to the direct sum S = sum_K |x||w| (K = taps * C), from the matrices:
    a transformed input element is a signed sum of at most b^2 inputs (b = max absolute row sum of B^T = 2), a transformed filter
    element at most g^2 times the largest filter element (g = max absolute row sum of G = 3/2 for F(2x2,3x3), 1 for F(3x3,2x2)'s dy
    transform), so a Winograd-domain product summed over the C channels (and, for the weight gradient, the tiles) is at most
    b^2 g^2 C |x||w|; the output transform then adds at most a^2 of them (a = max absolute row sum of A^T = 3).  Relative to
    S = taps * C |x||w| that is b^2 g^2 a^2 / taps.  The transformed filter carries two fractional bits (quarter-integers: G's entries
    are 0, +-1, +-1/2, applied twice), hence the tests demand  amplification * S < 2^22  — two bits below fp32's 2^24."""
    b = float(BT.abs().sum(1).max())
    g = float(G.abs().sum(1).max())
    a = float(AT.abs().sum(1).max())
    taps = G.shape[1] ** 2
    return b * b * g * g * a * a / taps


def wino_filter_image(w, flip=False):
    """w [n][3][3][c] (an OHWI filter, or a zsg_transpose_w image with flip: the filter rotated by 180 degrees for the data gradient)
    -> U [n][4][4][c] = G g G^T, exact quarter-integers"""
    g = w.to(DT)
    if flip:
        g = g.flip((1, 2))
    return torch.einsum("ia,nabc,jb->nijc", WINO_G, g, WINO_G)


# ---- operand builder ------------------------------------------------------------------------------------------------------------------
class Buf:
    """one flat fp32 buffer [GUARD | extent | GUARD]; `lo` elements more in front shift the body by that much (an `out` pointer that is
    not 16-byte aligned)"""

    def __init__(self, extent, fill, guard, shift=0):
        self.extent, self.shift = int(extent), shift
        self.t = torch.full((GUARD + shift + self.extent + GUARD,), float(guard), dtype=torch.float32)
        self.body.fill_(fill)

    @property
    def lo(self):
        return GUARD + self.shift

    @property
    def body(self):
        return self.t[self.lo:self.lo + self.extent]


def build_input(extent, idx, values, shift=0):
    """an input operand: NaN guards, poison inside the extent, `values` (float64 integers) at the addressed indices `idx`"""
    b = Buf(extent, POISON, float("nan"), shift)
    b.body[idx.reshape(-1)] = values.reshape(-1).float()
    return b


def build_output(extent, written, init=None, shift=0):
    """an output: SENTINEL in the guards and wherever the launch must not write, NaN (or `init`: the accumulate / aliased-add values)
    at the `written` indices"""
    b = Buf(extent, SENTINEL, SENTINEL, shift)
    b.body[written.reshape(-1)] = float("nan") if init is None else init.reshape(-1).float()
    return b


def expected_output(buf: Buf, ref_body, written):
    """the complete buffer (guards and sentinels included) a correct launch leaves behind"""
    e = buf.t.clone()
    e[buf.lo + written.reshape(-1)] = ref_body[written.reshape(-1)].float()
    return e


def rand_int(shape, amp, gen):
    """non-zero integers out of {+-1 .. +-amp}: every single product counts"""
    v = torch.randint(1, amp + 1, shape, generator=gen).to(DT)
    return v * (torch.randint(0, 2, shape, generator=gen).to(DT) * 2 - 1)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """one geometry + layout.  C: reduction channels of the forward (a multiple of 4), N: output channels.  Layout: source rows are
    src_ld wide, output rows out_ld; dy (weight / data gradient) rows dy_ld (= out_ld unless that is no multiple of 4: N = 45 lives
    in 48-wide rows there).  amp: operands are drawn from {+-1..+-amp}."""
    name: str
    B: int
    C: int
    N: int
    sizes: list
    k: int
    s: int = 1
    p: int = 0
    d: int = 1
    src_ld: Optional[int] = None
    out_ld: Optional[int] = None
    src_off: int = 0
    out_off: int = 0
    src_gap: int = 0
    out_gap: int = 0
    scatter: bool = False
    wC: Optional[int] = None
    wc0: int = 0
    wt_slack: int = 0
    merge_x: bool = False
    out_shift: int = 0            # the out pointer is this many elements off 16-byte alignment
    amp: int = 3
    amp_g: int = 3                # dy of the gradients
    wino: bool = False            # 3x3 / stride 1 / pad 1: also a Winograd geometry

    def __post_init__(self):
        self.src_ld = self.src_ld or self.C
        self.out_ld = self.out_ld or self.N
        self.wC = self.wC or self.C
        self.wt_ld = self.k * self.k * self.wC + self.wt_slack
        self.dy_ld = self.out_ld if self.out_ld % 4 == 0 else (self.N + 3) // 4 * 4
        self.wino = self.k == 3 and self.s == 1 and self.p == 1 and self.d == 1 and not self.merge_x
        self.osizes = [(conv_out(h, self.k, self.s, self.p, self.d), conv_out(w, self.k, self.s, self.p, self.d)) for h, w in self.sizes]

    def src_view(self):
        return make_view(self.B, self.C, self.sizes, self.src_ld, self.src_off, self.src_gap)

    def out_view(self, ld=None):
        ld = ld or self.out_ld
        return make_view(self.B, self.N, self.osizes, ld, self.out_off, self.out_gap, self.scatter)

    def fwd(self, relu=False):
        return fwd_desc(self.src_view(), self.out_view(), self.C, self.N, self.k, self.s, self.p, self.d, self.wC, self.wc0, self.wt_ld,
                        relu, self.merge_x)

    def wg(self):
        return fwd_desc(self.src_view(), self.out_view(self.dy_ld), self.C, self.N, self.k, self.s, self.p, self.d, self.wC, self.wc0,
                        self.wt_ld, False, self.merge_x)

    def dg(self):
        return dgrad_desc(self.out_view(self.dy_ld), self.src_view(), self.C, self.k, self.s, self.p, self.d)


PYR = [(10, 10), (5, 5), (3, 3), (1, 1)]

CASES = [
    Case("pw722", 2, 64, 64, [(19, 19)], 1),                                          # 722 rows: ragged against 64 and 128
    Case("pw9", 1, 64, 64, [(3, 3)], 1),                                              # 9 rows: fewer than any tile
    Case("pw256", 1, 128, 256, [(6, 7)], 1),                                          # every unit width of the streaming 1x1 kernel; two K chunks
    Case("c3", 2, 64, 128, [(20, 17)], 3, 1, 1, amp=2),                               # padding
    Case("c3s2", 2, 128, 128, [(21, 21)], 3, 2, 1, amp=2),                            # four dgrad parity classes, odd size
    Case("pws2", 3, 256, 64, [(9, 11)], 1, 2, 0),                                     # dgrad zero_fill
    Case("dil6", 1, 64, 96, [(12, 12)], 3, 1, 6, 6),                                  # dilation 6
    Case("c36", 2, 36, 72, [(7, 9)], 3, 1, 1),                                        # K tail of 32; Winograd's half chunk (C % 8 == 4)
    Case("c40", 2, 40, 72, [(7, 9)], 3, 1, 1),                                        # K tail of 32 / 64
    Case("n45", 2, 64, 45, [(10, 10)], 3, 1, 1),                                      # out_ld = 45: scalar epilogue; dy in 48-wide rows
    Case("k4644", 1, 516, 256, [(5, 5)], 3, 1, 1, amp=2),                             # K = 4644
    Case("head0", 1, 256, 256, [(5, 5)], 3, 1, 1, wC=516, wc0=0, amp=2),              # the head conv0 form: C = 256 inside wC = 516
    Case("wwin", 2, 64, 64, [(6, 7)], 3, 1, 1, wC=132, wc0=64, wt_slack=12),          # window offset and wt_ld slack
    Case("stem", 2, 4, 64, [(45, 37)], 7, 2, 3, merge_x=True),                        # the streaming first-layer kernel
    Case("stem_s", 1, 4, 64, [(7, 9)], 7, 2, 3, merge_x=True),                        # a window larger than the image
    Case("stem3", 2, 4, 64, [(13, 10)], 3, 1, 1, merge_x=True),                       # the 3x3 merge_x window
    Case("pyr64", 2, 64, 64, PYR, 3, 1, 1, scatter=True),                             # segments, level boundaries, single-pixel level
    Case("pyr45", 2, 64, 45, PYR, 3, 1, 1, scatter=True),
    Case("pad4", 2, 64, 64, [(9, 7)], 3, 1, 1, src_ld=72, out_ld=68, src_off=8, out_off=12, src_gap=24, out_gap=40),
    Case("pad8", 2, 64, 64, [(9, 7)], 1, 1, 0, src_ld=72, out_ld=72, src_off=4, out_off=8, src_gap=16, out_gap=32),
    Case("pyrpad", 2, 64, 64, PYR, 3, 1, 1, src_ld=72, out_ld=68, src_off=8, out_off=4, src_gap=8, out_gap=12),
    Case("unal", 2, 64, 64, [(6, 5)], 3, 1, 1, out_shift=1),                          # N % 4 == 0, the out pointer one element off
    Case("pwgap", 2, 64, 64, [(6, 5)], 1, src_gap=64, out_gap=64),                    # a 1x1 made non-dense by a batch-stride gap
]
CASE = {c.name: c for c in CASES}


class CaseData:
    """operand data and references of one case (computed once, shared, never modified)"""

    def __init__(self, c: Case, seed=0):
        self.c = c
        g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, c.name)))
        self.F, self.W, self.G = c.fwd(), c.wg(), c.dg()
        F, W, G = self.F, self.W, self.G
        # forward source and filter, flat (poison where not addressed)
        self.x_idx, self.w_idx = src_addressed(F), wt_index(F)
        self.x = torch.full((src_extent(F),), POISON, dtype=DT)
        self.x[self.x_idx] = rand_int((len(self.x_idx),), c.amp, g)
        self.w = torch.full((wt_extent(F),), POISON, dtype=DT)
        self.w[self.w_idx] = rand_int(tuple(self.w_idx.shape), c.amp, g)
        self.bias = rand_int((c.N,), 3, g)
        self.o_idx = out_written(F)
        self.add = torch.full((out_extent(F),), POISON, dtype=DT)
        self.add[self.o_idx] = rand_int((len(self.o_idx),), 3, g)
        self.mask = torch.full((out_extent(F),), POISON, dtype=DT)
        self.mask[self.o_idx] = rand_int((len(self.o_idx),), 1, g)
        # dy: N channels in dy_ld-wide rows.  For the weight gradient the pad lanes are not addressed (poison); for the data gradient
        # they are operand zeros (C_red = dy.ld)
        self.g_idx = out_written(W)
        gv = rand_int((len(self.g_idx),), c.amp_g, g)
        self.dy_w = torch.full((out_extent(W),), POISON, dtype=DT)
        self.dy_w[self.g_idx] = gv
        self.dy_d_idx = src_addressed(G)
        self.dy_d = torch.full((src_extent(G),), POISON, dtype=DT)
        self.dy_d[self.dy_d_idx] = 0
        self.dy_d[self.g_idx] = gv
        # WT[c][k][k][dy_ld]: the transposed dense filter window, pad columns zero
        wd = self.w[self.w_idx]                                                     # [N, k, k, C]
        wt = torch.zeros(c.C, c.k, c.k, c.dy_ld, dtype=DT)
        wt[..., :c.N] = wd.permute(3, 1, 2, 0)
        self.w_dense, self.wt = wd.contiguous(), wt
        self.dx_idx = out_written(G)
        self.prev = torch.full((out_extent(G),), POISON, dtype=DT)
        self.prev[self.dx_idx] = rand_int((len(self.dx_idx),), 3, g)
        self.dmask = torch.full((out_extent(G),), POISON, dtype=DT)
        self.dmask[self.dx_idx] = rand_int((len(self.dx_idx),), 1, g)
        self.dw_prev = rand_int(tuple(self.w_idx.shape), 3, g)
        self._cache = {}

    def memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def fwd_rows(self, mutate=None):
        return self.memo(("fr", mutate), lambda: conv_rows(self.F, self.x, self.w, mutate))

    def dg_rows(self, mutate=None):
        return self.memo(("dr", mutate), lambda: conv_rows(self.G, self.dy_d, self.wt.reshape(-1), mutate, self.c.N - 1))

    def dw(self, mutate=None):
        z = torch.zeros(wt_extent(self.W), dtype=DT)
        return self.memo(("dw", mutate), lambda: wgrad(self.W, self.x, self.dy_w, z, False, mutate)[self.w_idx])


_DATA = {}


def case_data(name) -> CaseData:
    if name not in _DATA:
        _DATA[name] = CaseData(CASE[name])
    return _DATA[name]


def pad0_neighbour_rows(cd: CaseData):
    """negative control: the forward of the NEIGHBOURING geometry — padding 0 instead of 1 on the same output grid (taps start at the
    output pixel itself) — which no correct result of the case may equal"""
    D = cd.c.fwd()
    for g in D.segs:
        g.ty.d0 = g.tx.d0 = 0
    return conv_rows(D, cd.x, cd.w)


def exactness(cd: CaseData):
    """the fp32 bounds of one case, from the reference alone: max over outputs of sum_K |x||w| (forward, data gradient, weight
    gradient), the largest column sum of squares of the forward output, the largest |value| any accumulate / add epilogue holds"""
    c, F, W, G = cd.c, cd.F, cd.W, cd.G
    ab = lambda D, a, b: max(float(r.max()) for r in conv_rows(D, a.abs(), b.abs()))
    zero = torch.zeros(wt_extent(W), dtype=DT)
    rows = torch.cat([r.reshape(-1, c.N) for r in cd.fwd_rows()])
    drows = [r for r in cd.dg_rows()]
    return {
        "fwd_abs": ab(F, cd.x, cd.w),
        "dgrad_abs": ab(G, cd.dy_d, cd.wt.reshape(-1)),
        "wgrad_abs": float(wgrad(W, cd.x.abs(), cd.dy_w.abs(), zero, False)[cd.w_idx].max()),
        "sumsq": float((rows * rows).sum(0).max()),
        "sum_abs": float(rows.abs().sum(0).max()),
        "fwd_epi": float(rows.abs().max()) + 3 + 3,
        "dgrad_epi": max(float(r.abs().max()) for r in drows) + 3,
        "wgrad_epi": float(cd.dw().abs().max()) + 3,
    }

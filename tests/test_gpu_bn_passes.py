"""The streaming half of csrc/bn.hip — the passes that walk [rows][C] data — through the C ABI at every block geometry, against the fp64
definitions of tests/bn_ref.py (proved on the CPU by tests/test_cpu_bn_ref.py).

Principle: exact data.  x, dout, residual, beta and mean are small integers, invstd and |gamma| powers of two in [0.25, 2], the free
backward coefficients multiples of 1/8, and every column sum of absolute values stays below 2^24 (bn_ref.check_exact asserts it for
every case).  Every intermediate is then a number fp32 holds, so summation order and FMA contraction excuse nothing and the comparison
is BIT equality: a dropped, repeated or misplaced row, channel group or mask byte always shows.  (ReLU outputs are compared after
`+ 0.0`, which leaves every bit but the sign of a zero: the ReLU rule fixes fmaxf(-0, 0) no further.)  The only two tolerances are on
the dx of zsg_bn_backward and zsg_bn_relu_maxpool_bwd, whose coefficients f32(se / rows), f32(sse / rows) are not dyadic: dbeta, dgamma
and the coefficients themselves are bit-exact, and dx is held to 1e-6 of |gamma * invstd| * (|g| + |c1| + |xhat * c2|), the seven
fp32 roundings of the expression (the bound of test_gpu_bn_finalize.test_backward_from_partials).  One test leaves the exact data:
test_apply_from_partials_second_batch reuses the integer partial rows and the checks of test_gpu_bn_finalize (mean bit-exact, invstd
within one ulp, out to 1e-6 of its terms), since eps = 1e-5 makes its invstd no dyadic number.  Every output is NaN (uint8: 255)
before the call and CANARY elements longer than needed; the tail must come back untouched.

Geometry (bn_geom): lanes = 1 .. 64 from C / 4, rowlanes = 256 / lanes, slabs = cdiv(C / 4, lanes), rpb = max(4 * rowlanes,
ceil(rows * slabs / 1024)).  GEOM = every C of {4, 8, 16, 32, 64, 128, 256 (lanes 1 .. 64), 12, 20, 260 (a last slab with one or two live
lanes), 2048 (8 slabs)} x rows of {1, rl - 1, rl, rl + 1, 4 rl - 1, 4 rl, 4 rl + 1 (a last chunk of one row), 9 rl + 3}, plus
(C, rows) = (4, 1 050 000), (64, 70 001), (256, 20 000), (2048, 2 500) where rpb grows past its floor (1026, 69, 20, 20).  Each test
first checks zsg_bn_workspace_bytes against the chunk count bn_ref.bn_geom predicts: should the kernels' geometry change, the tests say
that their edge cases need re-deriving.

Kernel, path, test:
  bn_partial_kernel<0>             GEOM; partial rows per chunk and fp64 sums      test_fwd_sums
  bn_partial_kernel<1>             GEOM; mask / none, accumulate 0 / 1             test_bwd_sums
                                   GEOM; relu_out gate / none (zsg_bn_backward)    test_backward_geom
                                   mask / relu_out / none x g_out x accumulate     test_backward_flags
  bn_apply_kernel                  GEOM; relu + residual + mask                    test_apply_geom
                                   relu x residual x mask cube, +0 / -0            test_apply_flags[plain]
                                   NaN, inf, denormals, +-0                        test_apply_special_values[plain]
  bn_apply_inl_kernel (body)       GEOM; one exact partial row                     test_apply_from_partials_geom
                                   flag cube                                       test_apply_flags[inline]
                                   prologue's second batch: C = 256 / 2048 with    test_apply_from_partials_second_batch
                                   32 / 33 / 64 partial rows
                                   special values                                  test_apply_special_values[inline]
  bn_bwd_apply_kernel              GEOM; dyadic coef, g_out NULL / given           test_bwd_apply_geom
                                   relu_out branch (zsg_bn_backward)               test_backward_geom, test_backward_flags
  bn_sync_bwd_apply_kernel         GEOM; fwd_sums[2C] = 8, sums = 8 coef: the      test_bwd_apply_geom
                                   bits of zsg_bn_bwd_apply
  bn_frozen_bwd_kernel<true>       GEOM; dx, g_out, dgamma, dbeta                  test_frozen_geom
                                   dx NULL, dgamma / dbeta / g_out only, mask      test_frozen_flags
  bn_frozen_bwd_kernel<false>      GEOM; the pure scale (x = mean = ws = NULL)     test_frozen_geom
                                   sums from given partial rows with x = NULL      test_frozen_flags
  bn_relu_maxpool_fwd_kernel       STEM grid, all windows, ties included           test_stem_fwd
                                   NaN taps, inf                                   test_stem_special_values
  bn_pool_bwd_partial_kernel       STEM grid (kmag at k = 15, cursors)             test_stem_sync_bwd, test_stem_bwd
  bn_sync_pool_bwd_apply_kernel    STEM grid, dyadic coefficients                  test_stem_sync_bwd
  bn_pool_bwd_apply_kernel         STEM grid, derived bound                        test_stem_bwd
  bn_frozen_pool_bwd_kernel<true>  STEM grid; dx given / NULL                      test_stem_frozen_bwd
  bn_frozen_pool_bwd_kernel<false> STEM grid                                       test_stem_frozen_bwd, test_stem_special_values
  every entry's ZSG_REQUIRE and workspace check                                    test_refusals
STEM grid: B in {1, 3} x C in {4, 20, 64} x (H, W) in {(1, 1), (1, 9), (7, 1), (13, 10)} x (k, s, p) in {(3, 2, 1), (2, 2, 0), (3, 1, 1),
(2, 3, 0): pixels in no window, (5, 3, 2), (15, 2, 7), (3, 2, 1) ceil mode}, wherever the padded image holds a window, plus
(B, H, W, C) = (2, 37, 41, 64) at (3, 2, 1) and (5, 3, 2): several chunks, cursors wrapping across image rows and images."""
import pytest
import torch

import bn_ref as R
import pointwise_ref as PR
from test_gpu_bn_finalize import EPS, MOM, check_stats, n_for, partials

pytestmark = pytest.mark.gpu

CANARY = 8
NAN = float("nan")
GEOM = R.geom_cases()
FLAG_GEOMS = [(20, 4 * 64 + 1), (260, 37)]
STEM = R.stem_cases()


def gid(v):
    return f"C{v[0]}-rows{v[1]}"


def sid(v):
    B, H, W, C, k, s, p, ceil = v
    return f"B{B}-{H}x{W}x{C}-k{k}s{s}p{p}{'ceil' if ceil else ''}"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as lib
    return lib


def fresh(n, dtype=torch.float32):
    """an output buffer of n elements plus the canary tail, every element NaN (uint8: 255)"""
    return torch.full((n + CANARY,), 255 if dtype == torch.uint8 else NAN, dtype=dtype, device="cuda")


def preload(t):
    buf = fresh(t.numel(), t.dtype)
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf


def untouched(t):
    return bool((t == 255).all() if t.dtype == torch.uint8 else torch.isnan(t).all())


def taken(buf, n):
    """the first n elements on the CPU, after checking the canary tail"""
    torch.cuda.synchronize()
    assert untouched(buf[n:].cpu()), "the kernel wrote past its output"
    return buf[:n].cpu()


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(got, want64, what, relu=False):
    """bit equality with the fp64 reference (every reference value is a number fp32 holds)"""
    got = got.reshape(-1)
    want = want64.reshape(-1).to(got.dtype)
    nan = torch.isnan(want)                                     # (special-value tests: a NaN is a NaN whatever its payload)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN at other positions than the reference's"
    got, want = got.masked_fill(nan, 0.0), want.masked_fill(nan, 0.0)
    assert torch.equal(want.double(), want64.reshape(-1).double().masked_fill(nan, 0.0)), f"{what}: the reference is not exact in fp32"
    if relu:
        got = got + 0.0
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}")


def f32_sum_ref(exact64, pre):
    """dgamma / dbeta as the kernels form them: the fp64 sum rounded to fp32 once, then (accumulate) one fp32 addition to what was there"""
    v = exact64.float()
    return v if pre is None else pre + v


def p(t):
    return None if t is None else t.data_ptr()


_DEV = {}


def dev(c):
    """the case's tensors on the GPU (copied once; no kernel writes to them)"""
    key = id(c)
    if key not in _DEV:
        _DEV[key] = {k: v.cuda() for k, v in c.items() if isinstance(v, torch.Tensor)}
    return _DEV[key]


def guard(L, rows, C):
    """the geometry guard: the workspace size follows from the chunk count bn_ref.bn_geom predicts"""
    wsb = int(L.lib.zsg_bn_workspace_bytes(rows, C))
    assert wsb == R.workspace_bytes(rows, C), (f"bn_geom({rows}, {C}) of csrc/bn.hip no longer gives {R.bn_geom(rows, C)}: the edge cases of this "
                                               "file were derived from that geometry and need re-deriving")
    return wsb


def chunk_sums(v64, rpb):
    """[rows, C] fp64 -> [chunks, C]: the sum of each block's rows"""
    rows, C = v64.shape
    chunks = -(-rows // rpb)
    pad = torch.zeros(chunks * rpb, C, dtype=torch.float64)
    pad[:rows] = v64
    return pad.view(chunks, rpb, C).sum(1)


def prior(C, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(-1000, 1001, (C,), generator=g).float() for _ in range(2))


def dx_bound_check(got_dx, dout_g, x, mean, invstd, gamma, c1, c2, what):
    """dx from the fp32 coefficients, to 1e-6 of the expression's terms |gamma invstd| (|g| + |c1| + |xhat c2|)"""
    sc = (invstd.double() * gamma.double()).abs()
    xh = R.xhat(x, mean, invstd)
    want = (invstd.double() * gamma.double()) * (dout_g - c1.double() - xh * c2.double())
    tol = 1e-6 * sc * (dout_g.abs() + c1.double().abs() + (xh * c2.double()).abs())
    err = (got_dx.double().view(want.shape) - want).abs()
    print(f"{what}: worst dx error / allowance {float((err / tol.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= tol).all()), f"{what}: dx, worst error / allowance {float((err / tol.clamp_min(1e-300)).max()):.3g}"


# ---- geometry grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_fwd_sums(L, C, rows):
    """bn_partial_kernel<0>: every block's partial row (sum x, sum x^2 of its rows) and the fp64 sums; sums[2C] = rows"""
    c, d, geo, wsb = R.case(rows, C), dev(R.case(rows, C)), R.bn_geom(rows, C), guard(L, rows, C)
    ws, sums = fresh(wsb // 4), fresh(2 * C + 1, torch.float64)
    L.check(L.lib.zsg_bn_sync_fwd_sums(p(d["x"]), rows, C, None, 0, p(sums), p(ws), wsb, L.stream_ptr()), "bn_sync_fwd_sums")
    x64 = c["x"].double()
    part = taken(ws, geo["chunks"] * 2 * C).view(geo["chunks"], 2, C)
    assert untouched(ws[geo["chunks"] * 2 * C:].cpu()), "the coefficient slots of the workspace are not this entry's to write"
    same(part[:, 0], chunk_sums(x64, geo["rpb"]), "partial rows, sum x")
    same(part[:, 1], chunk_sums(x64 * x64, geo["rpb"]), "partial rows, sum x^2")
    got = taken(sums, 2 * C + 1)
    same(got[:C], x64.sum(0), "sum x")
    same(got[C:2 * C], (x64 * x64).sum(0), "sum x^2")
    assert float(got[2 * C]) == rows


@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_bwd_sums(L, C, rows):
    """bn_partial_kernel<1> through zsg_bn_sync_bwd_sums: with and without mask, dgamma / dbeta at accumulate 0 and 1"""
    c, d, geo, wsb = R.case(rows, C), dev(R.case(rows, C)), R.bn_geom(rows, C), guard(L, rows, C)
    pre_g, pre_b = prior(C, rows + C)
    for g8 in ("mask", None):
        se, sse = R.backward_sums(c["dout"], c[g8] if g8 else None, c["x"], c["mean"], c["invstd"])
        g = R.gate(c["dout"], c[g8] if g8 else None)
        for acc in (0, 1):
            ws, sums = fresh(wsb // 4), fresh(2 * C, torch.float64)
            dg, db = (preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))
            L.check(L.lib.zsg_bn_sync_bwd_sums(p(d["dout"]), p(d[g8]) if g8 else None, p(d["x"]), rows, C, p(d["mean"]), p(d["invstd"]), None, 0,
                                               p(sums), p(dg), p(db), acc, p(ws), wsb, L.stream_ptr()), "bn_sync_bwd_sums")
            what = f"gate={g8} accumulate={acc}"
            got = taken(sums, 2 * C)
            same(got[:C], se, f"sum g, {what}")
            same(got[C:], sse, f"sum g xhat, {what}")
            same(taken(db, C), f32_sum_ref(se, pre_b if acc else None).double(), f"dbeta, {what}")
            same(taken(dg, C), f32_sum_ref(sse, pre_g if acc else None).double(), f"dgamma, {what}")
            if not acc:
                part = taken(ws, geo["chunks"] * 2 * C).view(geo["chunks"], 2, C)
                same(part[:, 0], chunk_sums(g, geo["rpb"]), f"partial rows, sum g, {what}")
                same(part[:, 1], chunk_sums(g * R.xhat(c["x"], c["mean"], c["invstd"]), geo["rpb"]), f"partial rows, sum g xhat, {what}")


def run_backward(L, c, d, g8, with_g_out, acc, pre_g, pre_b):
    """zsg_bn_backward with the gate `g8` ("mask", "relu_out" or None); checks everything it writes"""
    rows, C = c["rows"], c["C"]
    geo, wsb = R.bn_geom(rows, C), guard(L, rows, C)
    gate8 = c[g8] if g8 else None
    se, sse = R.backward_sums(c["dout"], gate8, c["x"], c["mean"], c["invstd"])
    ws, dx, g_out = fresh(wsb // 4), fresh(rows * C), (fresh(rows * C) if with_g_out else None)
    dg, db = (preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))
    L.check(L.lib.zsg_bn_backward(p(d["dout"]), p(d["relu_out"]) if g8 == "relu_out" else None, p(d["mask"]) if g8 == "mask" else None, p(d["x"]),
                                  rows, C, p(d["mean"]), p(d["invstd"]), p(d["gamma"]), p(dx), p(g_out), p(dg), p(db), acc, p(ws), wsb,
                                  L.stream_ptr()), "bn_backward")
    what = f"gate={g8} g_out={with_g_out} accumulate={acc}"
    same(taken(db, C), f32_sum_ref(se, pre_b if acc else None).double(), f"dbeta, {what}")
    same(taken(dg, C), f32_sum_ref(sse, pre_g if acc else None).double(), f"dgamma, {what}")
    coef = taken(ws, wsb // 4)[geo["chunks"] * 2 * C:]
    c1, c2 = (se / rows).float(), (sse / rows).float()
    same(coef[:C], c1.double(), f"coef 0 = f32(se / rows), {what}")
    same(coef[C:], c2.double(), f"coef 1 = f32(sse / rows), {what}")
    g = R.gate(c["dout"], gate8)
    if with_g_out:
        same(taken(g_out, rows * C), g, f"g_out, {what}")
    dx_bound_check(taken(dx, rows * C), g, c["x"], c["mean"], c["invstd"], c["gamma"], c1, c2, what)


@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_backward_geom(L, C, rows):
    """zsg_bn_backward with relu_out in place of the mask (only this entry reaches that branch of both kernels) and with neither"""
    c = R.case(rows, C)
    pre_g, pre_b = prior(C, rows * 3 + C)
    run_backward(L, c, dev(c), "relu_out", True, 0, pre_g, pre_b)
    run_backward(L, c, dev(c), None, False, 1, pre_g, pre_b)


def run_apply(L, c, d, relu, with_res, with_mask, inline, what):
    """zsg_bn_apply, or zsg_bn_apply_from_partials on ONE partial row built so that the statistics come out as the case's mean / invstd
    exactly (se = n mean, sse = n (1 / invstd^2 + mean^2), eps = 0: all exact in fp32 and fp64, asserted here)"""
    rows, C = c["rows"], c["C"]
    want, want_mask = R.apply(c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["residual"] if with_res else None, bool(relu))
    out, mask = fresh(rows * C), (fresh(rows * C // 4, torch.uint8) if with_mask else None)
    res = p(d["residual"]) if with_res else None
    if inline:
        mean, invstd, pd = fresh(C), fresh(C), R.exact_partial_row(rows, c["mean"], c["invstd"]).cuda()
        L.check(L.lib.zsg_bn_apply_from_partials(p(d["x"]), rows, C, p(pd), 1, p(d["gamma"]), p(d["beta"]), res, relu, p(out), p(mask), p(mean),
                                                 p(invstd), None, None, MOM, 0.0, L.stream_ptr()), "bn_apply_from_partials")
        same(taken(mean, C), c["mean"].double(), f"{what}: mean")
        same(taken(invstd, C), c["invstd"].double(), f"{what}: invstd")
    else:
        L.check(L.lib.zsg_bn_apply(p(d["x"]), rows, C, p(d["mean"]), p(d["invstd"]), p(d["gamma"]), p(d["beta"]), res, relu, p(out), p(mask),
                                   L.stream_ptr()), "bn_apply")
    got = taken(out, rows * C)
    same(got, want, f"{what}: out", relu=bool(relu))
    if with_mask:
        got_mask = taken(mask, rows * C // 4)
        if relu:
            assert torch.equal(got_mask, want_mask), f"{what}: mask bytes"
            assert int(got_mask.max()) < 16, f"{what}: bits 4-7 of a mask byte must be 0"
            assert bool((got.view(rows, C)[~R.unpack_mask(got_mask, rows, C)] == 0).all()), f"{what}: mask bit 0 but output not 0"
        else:
            assert untouched(got_mask), f"{what}: relu = 0 must leave the mask buffer alone"
    return want


@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_apply_geom(L, C, rows):
    c = R.case(rows, C)
    run_apply(L, c, dev(c), 1, True, True, False, "bn_apply")


@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_apply_from_partials_geom(L, C, rows):
    """the streaming body of bn_apply_inl_kernel at every geometry"""
    c = R.case(rows, C)
    run_apply(L, c, dev(c), 1, True, True, True, "bn_apply_from_partials")


@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_bwd_apply_geom(L, C, rows):
    """bn_bwd_apply_kernel with dyadic coefficients, g_out NULL and given; bn_sync_bwd_apply_kernel from fwd_sums[2C] = 8 and sums = 8 coef
    must give the same dx bits"""
    c, d = R.case(rows, C), dev(R.case(rows, C))
    guard(L, rows, C)
    want_dx, want_g = R.bwd_apply(c["dout"], c["mask"], c["x"], c["mean"], c["invstd"], c["gamma"], c["c1"], c["c2"])
    coef = torch.cat([c["c1"], c["c2"]]).cuda()
    sums = (torch.cat([c["c1"], c["c2"]]).double() * 8).cuda()
    fwd = torch.full((2 * C + 1,), NAN, dtype=torch.float64)
    fwd[2 * C] = 8
    fwd = fwd.cuda()
    for with_g_out in (False, True):
        for sync in (False, True):
            dx, g_out = fresh(rows * C), (fresh(rows * C) if with_g_out else None)
            if sync:
                L.check(L.lib.zsg_bn_sync_bwd_apply(p(d["dout"]), p(d["mask"]), p(d["x"]), rows, C, p(d["mean"]), p(d["invstd"]), p(d["gamma"]),
                                                    p(sums), p(fwd), p(dx), p(g_out), L.stream_ptr()), "bn_sync_bwd_apply")
            else:
                L.check(L.lib.zsg_bn_bwd_apply(p(d["dout"]), p(d["mask"]), p(d["x"]), rows, C, p(d["mean"]), p(d["invstd"]), p(d["gamma"]),
                                               p(coef), p(dx), p(g_out), L.stream_ptr()), "bn_bwd_apply")
            what = f"{'bn_sync_bwd_apply' if sync else 'bn_bwd_apply'} g_out={with_g_out}"
            same(taken(dx, rows * C), want_dx, f"dx, {what}")
            if with_g_out:
                same(taken(g_out, rows * C), want_g, f"g_out, {what}")
    # without a mask: g = dout
    dx = fresh(rows * C)
    L.check(L.lib.zsg_bn_bwd_apply(p(d["dout"]), None, p(d["x"]), rows, C, p(d["mean"]), p(d["invstd"]), p(d["gamma"]), p(coef), p(dx), None,
                                   L.stream_ptr()), "bn_bwd_apply")
    same(taken(dx, rows * C), R.bwd_apply(c["dout"], None, c["x"], c["mean"], c["invstd"], c["gamma"], c["c1"], c["c2"])[0], "dx, no mask")


def run_frozen(L, c, d, what, mask=True, x=True, dx=True, g_out=False, dgamma=False, dbeta=False, acc=0, part=None):
    """zsg_bn_frozen_backward with the named pointers given and every other one NULL; checks what it writes and that nothing else is"""
    rows, C = c["rows"], c["C"]
    geo = R.bn_geom(rows, C)
    ref = R.frozen_backward(c["dout"], c["mask"] if mask else None, c["x"], c["mean"], c["invstd"], c["gamma"])
    sums = dgamma or dbeta
    own = sums and part is None
    wsb = guard(L, rows, C) if own else (2 * C * 4 if sums else 0)
    pre_g, pre_b = prior(C, rows * 5 + C)
    b_dx, b_g = (fresh(rows * C) if dx else None), (fresh(rows * C) if g_out else None)
    b_dg = (preload(pre_g) if acc else fresh(C)) if dgamma else None
    b_db = (preload(pre_b) if acc else fresh(C)) if dbeta else None
    ws = fresh(wsb // 4) if sums else None
    pd = part.cuda() if part is not None else None
    L.check(L.lib.zsg_bn_frozen_backward(p(d["dout"]), p(d["mask"]) if mask else None, p(d["x"]) if x else None, rows, C,
                                         p(d["mean"]) if x else None, p(d["invstd"]), p(d["gamma"]), p(b_dx), p(b_g), p(b_dg), p(b_db), acc, p(pd),
                                         part.shape[0] if part is not None else 0, p(ws), wsb, L.stream_ptr()), "bn_frozen_backward")
    if dx:
        same(taken(b_dx, rows * C), ref["dx"], f"{what}: dx")
    if g_out:
        same(taken(b_g, rows * C), ref["g"], f"{what}: g_out")
    if part is not None:
        ref["dbeta"], ref["dgamma"] = PR.bn_partial_sums(part)
    if dbeta:
        same(taken(b_db, C), f32_sum_ref(ref["dbeta"], pre_b if acc else None).double(), f"{what}: dbeta")
    if dgamma:
        same(taken(b_dg, C), f32_sum_ref(ref["dgamma"], pre_g if acc else None).double(), f"{what}: dgamma")
    if own:
        rows_part = taken(ws, wsb // 4)[:geo["chunks"] * 2 * C].view(geo["chunks"], 2, C)
        same(rows_part[:, 0], chunk_sums(ref["g"], geo["rpb"]), f"{what}: partial rows, sum g")
        same(rows_part[:, 1], chunk_sums(ref["g"] * R.xhat(c["x"], c["mean"], c["invstd"]), geo["rpb"]), f"{what}: partial rows, sum g xhat")
    elif sums:
        taken(ws, 2 * C)                          # (2 C coefficient slots, the finalize kernel's: no more)


@pytest.mark.parametrize("C,rows", GEOM, ids=map(gid, GEOM))
def test_frozen_geom(L, C, rows):
    """bn_frozen_bwd_kernel<true> (dx, g_out, dgamma, dbeta in one pass) and <false> as the pure scale dx = gamma invstd dout with
    x = mean = dgamma = dbeta = ws = NULL and no mask"""
    c = R.case(rows, C)
    run_frozen(L, c, dev(c), "all outputs", g_out=True, dgamma=True, dbeta=True)
    run_frozen(L, c, dev(c), "pure scale", mask=False, x=False)


# ---- pointer and flag combinations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inline", [False, True], ids=["plain", "inline"])
@pytest.mark.parametrize("C,rows", FLAG_GEOMS, ids=map(gid, FLAG_GEOMS))
def test_apply_flags(L, C, rows, inline):
    """relu x residual x mask.  The data hold values that normalise to exactly +0 (channel 0) and -0 (channel 1): without ReLU both signs
    come back bit for bit; with it the mask bit is 0 and the output 0"""
    c = R.case(rows, C)
    for relu in (0, 1):
        for with_res in (False, True):
            for with_mask in (False, True):
                want = run_apply(L, c, dev(c), relu, with_res, with_mask, inline, f"relu={relu} residual={with_res} mask={with_mask}")
                if not with_res and not relu:
                    z = want[::3, :2]
                    assert bool((z == 0).all()) and not bool(torch.signbit(z[:, 0]).any()) and bool(torch.signbit(z[:, 1]).all())


@pytest.mark.parametrize("C", [256, 2048])
@pytest.mark.parametrize("chunks", [32, 33, 64])
def test_apply_from_partials_second_batch(L, chunks, C):
    """bn_apply_inl_kernel's prologue takes 8 partial rows per row lane and batch: with the 4 row lanes of C >= 256, 33 and 64 integer rows
    (the construction of test_gpu_bn_finalize) make its second batch run, 32 is the last count without.  Statistics as that file checks
    them; out from the kernel's own statistics to 1e-6 of its two terms (four fp32 roundings)."""
    assert R.bn_geom(64, C)["rowlanes"] == 4 and chunks <= int(L.lib.zsg_bn_inline_max_chunks())
    part, se, sse = partials(chunks, C)
    rows = n_for(max(chunks, 64))
    g = torch.Generator().manual_seed(chunks * 7 + C)
    x = torch.randn(rows, C, generator=g) * 30
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g) * 100, torch.rand(C, generator=g) * 1e5 + 1
    ref = PR.bn_finalize(se, sse, rows, EPS, rm0, rv0, MOM)
    pd, xd, gd, bd = (t.cuda() for t in (part, x, gamma, beta))
    out, mean, invstd, rm, rv = fresh(rows * C), fresh(C), fresh(C), preload(rm0), preload(rv0)
    L.check(L.lib.zsg_bn_apply_from_partials(p(xd), rows, C, p(pd), chunks, p(gd), p(bd), None, 0, p(out), None, p(mean), p(invstd), p(rm), p(rv),
                                             MOM, EPS, L.stream_ptr()), "bn_apply_from_partials")
    got_mean, got_invstd = taken(mean, C), taken(invstd, C)
    check_stats(got_mean, got_invstd, taken(rm, C), taken(rv, C), ref, f"chunks={chunks}")
    sc = got_invstd * gamma
    want = (x - got_mean) * sc + beta
    err = (taken(out, rows * C).view(rows, C).double() - want.double()).abs()
    assert bool((err <= 1e-6 * (((x - got_mean) * sc).abs() + beta.abs()).double()).all()), f"out off by {float(err.max()):.3g}"


@pytest.mark.parametrize("C,rows", FLAG_GEOMS, ids=map(gid, FLAG_GEOMS))
def test_backward_flags(L, C, rows):
    c = R.case(rows, C)
    pre_g, pre_b = prior(C, rows * 7 + C)
    for g8 in ("mask", "relu_out", None):
        for with_g_out in (False, True):
            for acc in (0, 1):
                run_backward(L, c, dev(c), g8, with_g_out, acc, pre_g, pre_b)


@pytest.mark.parametrize("C,rows", FLAG_GEOMS, ids=map(gid, FLAG_GEOMS))
def test_frozen_flags(L, C, rows):
    c, d = R.case(rows, C), dev(R.case(rows, C))
    for mask in (False, True):
        run_frozen(L, c, d, f"pure scale, mask={mask}", mask=mask, x=False)
        run_frozen(L, c, d, f"dx NULL with sums, mask={mask}", mask=mask, dx=False, dgamma=True, dbeta=True, acc=1)
        run_frozen(L, c, d, f"dgamma only, mask={mask}", mask=mask, dgamma=True)
        run_frozen(L, c, d, f"dbeta only, mask={mask}", mask=mask, dbeta=True, acc=1)
        run_frozen(L, c, d, f"g_out only, mask={mask}", mask=mask, dx=False, g_out=True)
        part, _, _ = partials(33, 64)
        part = part[:, :, :1].expand(33, 2, C).contiguous() + torch.arange(C).float()
        run_frozen(L, c, d, f"sums from partial rows, x NULL, mask={mask}", mask=mask, x=False, dgamma=True, dbeta=True, part=part)
        run_frozen(L, c, d, f"sums from partial rows alone, mask={mask}", mask=mask, x=False, dx=False, dbeta=True, acc=1, part=part)


# ---- stem ----------------------------------------------------------------------------------------------------------------------------
def stem_args(c, d):
    return [c["B"], c["H"], c["W"], c["C"], p(d["mean"]), p(d["invstd"]), p(d["gamma"]), p(d["beta"]), c["k"], c["s"], c["p"], c["Ho"], c["Wo"]]


@pytest.mark.parametrize("key", STEM, ids=map(sid, STEM))
def test_stem_fwd(L, key):
    """out and idx for ALL windows: on this data most windows tie (at the ReLU's 0 above all), and the first in-bounds tap must win"""
    c = R.stem_case(*key)
    d = dev(c)
    n = c["out"].numel()
    out, idx = fresh(n), fresh(n, torch.uint8)
    L.check(L.lib.zsg_bn_relu_maxpool_fwd(p(d["x"]), *stem_args(c, d), p(out), p(idx), L.stream_ptr()), "bn_relu_maxpool_fwd")
    same(taken(out, n), c["out"], "out", relu=True)
    got = taken(idx, n)
    want = c["idx"].reshape(-1)
    assert torch.equal(got, want), f"idx: {int((got != want).sum())} of {n} windows differ ({int((c['out'] == 0).sum())} windows hold only zeros)"


@pytest.mark.parametrize("key", STEM, ids=map(sid, STEM))
def test_stem_sync_bwd(L, key):
    """bn_pool_bwd_partial_kernel's fp64 sums, dgamma / dbeta at accumulate 0 and 1; bn_sync_pool_bwd_apply_kernel with fwd_sums[2C] = 8
    and sums = 8 coef (dyadic coefficients): exact dx"""
    c = R.stem_case(*key)
    d = dev(c)
    B, H, W, C, k, s, pp = c["B"], c["H"], c["W"], c["C"], c["k"], c["s"], c["p"]
    prow, rows = B * c["Ho"] * c["Wo"], B * H * W
    wsb = guard(L, prow, C)
    guard(L, rows, C)
    se, sse = R.stem_backward_sums(c["dout"], c["idx"], c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], k, s, pp)
    pre_g, pre_b = prior(C, rows + C)
    for acc in (0, 1):
        ws, sums = fresh(wsb // 4), fresh(2 * C, torch.float64)
        dg, db = (preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))
        L.check(L.lib.zsg_bn_sync_relu_maxpool_bwd_sums(p(d["dout"]), p(d["idx"]), p(d["x"]), *stem_args(c, d), p(sums), p(dg), p(db), acc, p(ws),
                                                        wsb, L.stream_ptr()), "bn_sync_relu_maxpool_bwd_sums")
        got = taken(sums, 2 * C)
        taken(ws, wsb // 4)
        same(got[:C], se, f"sum g, accumulate={acc}")
        same(got[C:], sse, f"sum g xhat, accumulate={acc}")
        same(taken(db, C), f32_sum_ref(se, pre_b if acc else None).double(), f"dbeta, accumulate={acc}")
        same(taken(dg, C), f32_sum_ref(sse, pre_g if acc else None).double(), f"dgamma, accumulate={acc}")
    sums = (torch.cat([c["c1"], c["c2"]]).double() * 8).cuda()
    fwd = torch.full((2 * C + 1,), NAN, dtype=torch.float64)
    fwd[2 * C] = 8
    fwd = fwd.cuda()
    dx = fresh(rows * C)
    L.check(L.lib.zsg_bn_sync_relu_maxpool_bwd_apply(p(d["dout"]), p(d["idx"]), p(d["x"]), *stem_args(c, d), p(sums), p(fwd), p(dx),
                                                     L.stream_ptr()), "bn_sync_relu_maxpool_bwd_apply")
    same(taken(dx, rows * C), R.stem_bwd_apply(c["dout"], c["idx"], c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], k, s, pp, c["c1"],
                                               c["c2"]), "dx")


@pytest.mark.parametrize("key", STEM, ids=map(sid, STEM))
def test_stem_frozen_bwd(L, key):
    """bn_frozen_pool_bwd_kernel<true> with dx given and NULL, <false> (no sums): exact dx, dgamma, dbeta"""
    c = R.stem_case(*key)
    d = dev(c)
    C, rows = c["C"], c["B"] * c["H"] * c["W"]
    wsb = guard(L, rows, C)
    ref = R.stem_frozen_backward(c["dout"], c["idx"], c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["k"], c["s"], c["p"])
    pre_g, pre_b = prior(C, rows * 3 + C)
    for with_dx, with_sums, acc in ((True, True, 0), (False, True, 1), (True, False, 0)):
        dx = fresh(rows * C) if with_dx else None
        dg, db = ((preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))) if with_sums else (None, None)
        ws = fresh(wsb // 4) if with_sums else None
        L.check(L.lib.zsg_bn_frozen_relu_maxpool_bwd(p(d["dout"]), p(d["idx"]), p(d["x"]), *stem_args(c, d), p(dx), p(dg), p(db), acc, p(ws),
                                                     wsb if with_sums else 0, L.stream_ptr()), "bn_frozen_relu_maxpool_bwd")
        what = f"dx={with_dx} sums={with_sums} accumulate={acc}"
        if with_dx:
            same(taken(dx, rows * C), ref["dx"], f"dx, {what}")
        if with_sums:
            taken(ws, wsb // 4)
            same(taken(db, C), f32_sum_ref(ref["dbeta"], pre_b if acc else None).double(), f"dbeta, {what}")
            same(taken(dg, C), f32_sum_ref(ref["dgamma"], pre_g if acc else None).double(), f"dgamma, {what}")


@pytest.mark.parametrize("key", STEM, ids=map(sid, STEM))
def test_stem_bwd(L, key):
    """zsg_bn_relu_maxpool_bwd: dbeta = f32(se), dgamma = f32(sse), the coefficients f32(se / rows), f32(sse / rows) with rows = B H W, all
    bit for bit; dx to the derived bound"""
    c = R.stem_case(*key)
    d = dev(c)
    C, k, s, pp = c["C"], c["k"], c["s"], c["p"]
    prow, rows = c["B"] * c["Ho"] * c["Wo"], c["B"] * c["H"] * c["W"]
    wsb = guard(L, prow, C)
    se, sse = R.stem_backward_sums(c["dout"], c["idx"], c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], k, s, pp)
    pre_g, pre_b = prior(C, rows * 5 + C)
    g = R.stem_gather(c["dout"], c["idx"], c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], k, s, pp)
    for acc in (0, 1):
        ws, dx = fresh(wsb // 4), fresh(rows * C)
        dg, db = (preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))
        L.check(L.lib.zsg_bn_relu_maxpool_bwd(p(d["dout"]), p(d["idx"]), p(d["x"]), *stem_args(c, d), p(dx), p(dg), p(db), acc, p(ws), wsb,
                                              L.stream_ptr()), "bn_relu_maxpool_bwd")
        same(taken(db, C), f32_sum_ref(se, pre_b if acc else None).double(), f"dbeta, accumulate={acc}")
        same(taken(dg, C), f32_sum_ref(sse, pre_g if acc else None).double(), f"dgamma, accumulate={acc}")
        coef = taken(ws, wsb // 4)[R.bn_geom(prow, C)["chunks"] * 2 * C:]
        c1, c2 = (se / rows).float(), (sse / rows).float()
        same(coef[:C], c1.double(), "coef 0 = f32(se / rows)")
        same(coef[C:], c2.double(), "coef 1 = f32(sse / rows)")
        dx_bound_check(taken(dx, rows * C), g, c["x"], c["mean"], c["invstd"], c["gamma"], c1, c2, f"accumulate={acc}")


# ---- special values ----------------------------------------------------------------------------------------------------------------------
INF = float("inf")
TINY = 2.0 ** -140          # an fp32 denormal


@pytest.mark.parametrize("inline", [False, True], ids=["plain", "inline"])
def test_apply_special_values(L, inline):
    """mean = 0, invstd = gamma = 1, beta = 0.  With relu a NaN gives output 0 and mask bit 0 (fmaxf: the rule of zsg_relu_fwd), and so does
    inf + -inf through the residual; without relu the NaN stays.  +-inf, denormals and zeros pass as IEEE arithmetic has them."""
    rows, C = 3, 8
    x = torch.tensor([[NAN, 1.0, -0.0, INF, -INF, 0.0, TINY, -TINY], [INF, INF, NAN, -1.0, TINY, -INF, 2.0, -0.0],
                      [-TINY, NAN, 3.0, -3.0, INF, 0.0, -0.0, TINY]])
    res = torch.tensor([[1.0, NAN, 0.0, -INF, INF, -0.0, -TINY, TINY], [0.0, 1.0, 1.0, 1.0, TINY, 5.0, NAN, 0.0],
                        [2 * TINY, NAN, -3.0, 3.0, INF, 0.0, 0.0, -TINY]])
    zero, one = torch.zeros(C), torch.ones(C)
    c = {"rows": rows, "C": C, "x": x, "residual": res, "mean": zero, "invstd": one, "gamma": one, "beta": zero}
    d = {k: v.cuda() for k, v in c.items() if isinstance(v, torch.Tensor)}
    for with_res in (False, True):
        want = run_apply(L, c, d, 1, with_res, True, inline, f"relu=1 residual={with_res}")
        v = x.double() + (res.double() if with_res else 0)
        assert bool((want[torch.isnan(v)] == 0).all()) and int(torch.isnan(v).sum()) >= 3 and not bool(torch.isnan(want).any())
        kept = run_apply(L, c, d, 0, with_res, False, inline, f"relu=0 residual={with_res}")
        assert torch.equal(torch.isnan(kept), torch.isnan(v))
    # backward: the NaN positions carry mask bit 0, so g = 0 there
    _, mask = R.apply(x, zero, one, one, zero, None, True)
    dout = torch.arange(1, rows * C + 1).float().view(rows, C)
    g_out, dd, md = fresh(rows * C), dout.cuda(), mask.cuda()
    L.check(L.lib.zsg_bn_frozen_backward(p(dd), p(md), None, rows, C, None, p(d["invstd"]), p(d["gamma"]), None, p(g_out), None,
                                         None, 0, None, 0, None, 0, L.stream_ptr()), "bn_frozen_backward")
    got = taken(g_out, rows * C).view(rows, C)
    assert bool((got[torch.isnan(x)] == 0).all())
    same(got, R.gate(dout, mask), "g_out")


def test_stem_special_values(L):
    """a NaN tap counts as 0 (the ReLU's fmaxf comes before the comparison) and does not propagate; a window of NaN alone gives 0 at its
    first tap; inf wins; in the backward a NaN position passes no gradient"""
    B, H, W, C, k, s, pp = 1, 4, 4, 4, 2, 2, 0
    x = torch.tensor([[NAN, -1.0, NAN, 2.0], [3.0, NAN, NAN, NAN], [NAN, NAN, INF, -INF], [1.0, NAN, NAN, TINY]]).repeat(4, 1).view(B, H, W, C).clone()
    x[0, 2:, 2:] = NAN                                                       # the last window: NaN alone
    zero, one = torch.zeros(C), torch.ones(C)
    want_out, want_idx = R.stem_fwd(x, zero, one, one, zero, k, s, pp, 2, 2)
    assert not bool(torch.isnan(want_out).any()) and float(want_out[0, 1, 1].abs().sum()) == 0 and int(want_idx[0, 1, 1].sum()) == 0
    xd, zd, od = x.cuda(), zero.cuda(), one.cuda()
    args = [B, H, W, C, p(zd), p(od), p(od), p(zd), k, s, pp, 2, 2]
    out, idx = fresh(16), fresh(16, torch.uint8)
    L.check(L.lib.zsg_bn_relu_maxpool_fwd(p(xd), *args, p(out), p(idx), L.stream_ptr()), "bn_relu_maxpool_fwd")
    same(taken(out, 16), want_out, "out", relu=True)
    assert torch.equal(taken(idx, 16), want_idx.reshape(-1))
    dout = torch.arange(1, 17).float().view(1, 2, 2, 4)
    dx, dd, idd = fresh(B * H * W * C), dout.cuda(), want_idx.cuda()
    L.check(L.lib.zsg_bn_frozen_relu_maxpool_bwd(p(dd), p(idd), p(xd), *args, p(dx), None, None, 0, None, 0, L.stream_ptr()),
            "bn_frozen_relu_maxpool_bwd")
    got = taken(dx, B * H * W * C).view(B, H, W, C)
    assert bool((got[torch.isnan(x)] == 0).all())
    same(got, R.stem_gather(dout, want_idx, x, zero, one, one, zero, k, s, pp), "dx")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
BN = "B H W C mean invstd gamma beta k s p Ho Wo".split()
ENTRIES = {     # entry: (parameters in order, the one that counts rows, a required pointer, has a workspace check)
    "zsg_bn_sync_fwd_sums": ("x rows C null zero sums64 ws ws_bytes".split(), "rows", "sums64", True),
    "zsg_bn_sync_bwd_sums": ("dout mask x rows C mean invstd null zero sums64 dgamma dbeta zero ws ws_bytes".split(), "rows", "invstd", True),
    "zsg_bn_sync_bwd_apply": ("dout mask x rows C mean invstd gamma sums_in fwd_in dx g_out".split(), "rows", "fwd_in", False),
    "zsg_bn_apply": ("x rows C mean invstd gamma beta residual one out mask_out".split(), "rows", "out", False),
    "zsg_bn_apply_from_partials": ("x rows C part one gamma beta residual one out mask_out mean_out invstd_out null null mom eps".split(), "rows",
                                   "part", False),
    "zsg_bn_bwd_apply": ("dout mask x rows C mean invstd gamma coef dx g_out".split(), "rows", "coef", False),
    "zsg_bn_backward": ("dout null mask x rows C mean invstd gamma dx g_out dgamma dbeta zero ws ws_bytes".split(), "rows", "dx", True),
    "zsg_bn_frozen_backward": ("dout mask x rows C mean invstd gamma dx g_out dgamma dbeta zero null zero ws ws_bytes".split(), "rows", "gamma", True),
    "zsg_bn_relu_maxpool_fwd": (["sx"] + BN + ["sout", "sidx"], "B", "sidx", False),
    "zsg_bn_relu_maxpool_bwd": (["sdout", "sidx_in", "sx"] + BN + "sdx dgamma dbeta zero sws sws_bytes".split(), "B", "sdx", True),
    "zsg_bn_frozen_relu_maxpool_bwd": (["sdout", "sidx_in", "sx"] + BN + "sdx dgamma dbeta zero fws fws_bytes".split(), "B", "beta", True),
    "zsg_bn_sync_relu_maxpool_bwd_sums": (["sdout", "sidx_in", "sx"] + BN + "sums64 dgamma dbeta zero sws sws_bytes".split(), "B", "sums64", True),
    "zsg_bn_sync_relu_maxpool_bwd_apply": (["sdout", "sidx_in", "sx"] + BN + "sums_in fwd_in sdx".split(), "B", "fwd_in", False),
}


def test_refusals(L):
    """every entry: C % 4 != 0, no rows, a missing required pointer -> -1 and zsg_last_error names the entry; a workspace one byte short
    -> -2; nothing is written by any of them"""
    rows, C, B, H, W, k, s, pp, Ho, Wo = 5, 8, 1, 4, 4, 3, 2, 1, 2, 2
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    outs = {"sums64": fresh(2 * C + 1, torch.float64), "dgamma": fresh(C), "dbeta": fresh(C), "dx": fresh(rows * C), "g_out": fresh(rows * C),
            "out": fresh(rows * C), "mask_out": fresh(rows * C // 4, torch.uint8), "mean_out": fresh(C), "invstd_out": fresh(C),
            "sout": fresh(B * Ho * Wo * C), "sidx": fresh(B * Ho * Wo * C, torch.uint8), "sdx": fresh(B * H * W * C),
            "ws": fresh(64 * C), "sws": fresh(64 * C), "fws": fresh(64 * C)}
    ins = {"x": z(rows * C), "dout": z(rows * C), "residual": z(rows * C), "mask": z(rows * C // 4, torch.uint8), "mean": z(C), "invstd": z(C) + 1,
           "gamma": z(C) + 1, "beta": z(C), "coef": z(2 * C), "part": z(2 * C), "sums_in": z(2 * C, torch.float64),
           "fwd_in": z(2 * C + 1, torch.float64) + 1, "sx": z(B * H * W * C), "sdout": z(B * Ho * Wo * C), "sidx_in": z(B * Ho * Wo * C, torch.uint8)}
    vals = {k_: v.data_ptr() for k_, v in {**outs, **ins}.items()}
    vals.update(rows=rows, C=C, B=B, H=H, W=W, k=k, s=s, p=pp, Ho=Ho, Wo=Wo, null=None, zero=0, one=1, mom=MOM, eps=EPS,
                ws_bytes=int(L.lib.zsg_bn_workspace_bytes(rows, C)), sws_bytes=int(L.lib.zsg_bn_workspace_bytes(B * Ho * Wo, C)),
                fws_bytes=int(L.lib.zsg_bn_workspace_bytes(B * H * W, C)))
    for entry, (names, rows_name, required, has_ws) in ENTRIES.items():
        fn = getattr(L.lib, entry)
        ws_name = next((n for n in names if n.endswith("ws_bytes")), None)
        trials = [({"C": 6}, -1), ({rows_name: 0}, -1), ({required: None}, -1)] + ([({ws_name: vals[ws_name] - 1}, -2)] if has_ws else [])
        for over, want_rc in trials:
            rc = fn(*[over.get(n, vals[n]) for n in names], L.stream_ptr())
            assert rc == want_rc, f"{entry} with {over}: rc = {rc}"
            assert entry[4:].encode() in L.lib.zsg_last_error(), f"{entry} with {over}: {L.lib.zsg_last_error()}"
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert untouched(buf.cpu()), f"a refused call wrote to {name}"

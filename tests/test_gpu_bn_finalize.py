"""The finalize half of csrc/bn.hip (bn_reduce_partials and its callers) on synthetic partial rows, through the C ABI, against the fp64
finalize of tests/pointwise_ref.py.  No convolution runs: the [chunks][2][C] partial rows are plain data.

The rows hold integers (first half, "sum e": uniform in [-1000, 1000]; second half, "sum e^2": distinct values of [0, 2^20)) and the
row count n is a power of two >= chunks, so the fp64 column sums and se / n are exact whatever order the kernel adds in: a dropped,
repeated or misplaced partial row always changes the result.  `chunks` sits on every boundary of the reduction: its step of
64 lanes x 4 waves x 3 rows = 768 (767 / 768 / 769, 1535 / 1536 / 1537), the switch to 16 waves above 1536 rows and that form's step of
3072 (3071 / 3072 / 3073), one wave's worth (255 / 256 / 257) and the stem's 5625 rows of the benchmark shape."""
import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

CANARY = 8
NAN = float("nan")
CHUNKS = [1, 2, 255, 256, 257, 767, 768, 769, 1535, 1536, 1537, 3071, 3072, 3073, 5625]
CHANNELS = [4, 8, 64]
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as lib
    return lib


def fresh(n, dtype=torch.float32):
    return torch.full((n + CANARY,), NAN, dtype=dtype, device="cuda")


def preload(t):
    buf = fresh(t.numel(), t.dtype)
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf


def taken(buf, n):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:].cpu()).all()), "the kernel wrote past its output"
    return buf[:n].cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def n_for(chunks):
    """the row count: a power of two >= chunks (and >= 2, so the unbiased factor n / (n - 1) is in play)"""
    n = 2
    while n < chunks:
        n *= 2
    return n


_PARTIALS = {}


def partials(chunks, C):
    """[chunks][2][C] integer partial rows (made once per shape, never modified) and their fp64 column sums"""
    key = (chunks, C)
    if key not in _PARTIALS:
        g = torch.Generator().manual_seed(chunks * 131 + C)
        part = torch.empty(chunks, 2, C)
        part[:, 0] = torch.randint(-1000, 1001, (chunks, C), generator=g).float()
        part[:, 1] = torch.randperm(1 << 20, generator=g)[:chunks * C].view(chunks, C).float()
        _PARTIALS[key] = (part, *R.bn_partial_sums(part))
    return _PARTIALS[key]


def run_stats(L, part_dev, chunks, n, C, rm0=None, rv0=None):
    mean, invstd = fresh(C), fresh(C)
    rm = preload(rm0) if rm0 is not None else None
    rv = preload(rv0) if rv0 is not None else None
    L.check(L.lib.zsg_bn_stats_from_partials(part_dev.data_ptr(), chunks, n, C, mean.data_ptr(), invstd.data_ptr(),
                                             rm.data_ptr() if rm is not None else None, rv.data_ptr() if rv is not None else None, MOM, EPS,
                                             L.stream_ptr()), "bn_stats_from_partials")
    return taken(mean, C), taken(invstd, C), (taken(rm, C) if rm is not None else None), (taken(rv, C) if rv is not None else None)


def check_stats(got_mean, got_invstd, got_rm, got_rv, ref, what):
    assert torch.equal(bits(got_mean), bits(ref["mean"])), f"{what}: mean is not f32(se / n)"
    # invstd: one fp32 unit — the fp64 `sse / n - m * m` may contract to an FMA, the only freedom before the final rounding
    assert int(R.ulp_distance(got_invstd, ref["invstd"]).max()) <= 1, f"{what}: invstd off by more than one ulp"
    # running statistics: (1 - mom) * old + mom * new in fp32 = three roundings of 2^-24 each, rounded up to 2^-22 of the two terms
    for got, key, terms in ((got_rm, "running_mean", "rm_terms"), (got_rv, "running_var", "rv_terms")):
        if got is not None:
            a, b = ref[terms]
            err = (got.double() - ref[key]).abs()
            assert bool((err <= 2.0 ** -22 * (a.abs() + b.abs())).all()), f"{what}: {key} off by {float(err.max()):.3g}"


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("chunks", CHUNKS)
def test_stats_from_partials(L, chunks, C):
    part, se, sse = partials(chunks, C)
    n = n_for(chunks)
    g = torch.Generator().manual_seed(chunks + C)
    rm0, rv0 = torch.randn(C, generator=g) * 100, torch.rand(C, generator=g) * 1e5 + 1
    ref = R.bn_finalize(se, sse, n, EPS, rm0, rv0, MOM)
    check_stats(*run_stats(L, part.cuda(), chunks, n, C, rm0, rv0), ref, f"chunks={chunks}")
    m2, i2, _, _ = run_stats(L, part.cuda(), chunks, n, C)                    # without running statistics: the same bits
    assert torch.equal(bits(m2), bits(ref["mean"])) and int(R.ulp_distance(i2, ref["invstd"]).max()) <= 1


@pytest.mark.parametrize("chunks", CHUNKS)
def test_stats_single_nonzero_row(L, chunks):
    """exactly one non-zero partial row, placed on each side of every loop / wave boundary: the mean must be that value over n, exactly"""
    C = 8
    n = n_for(chunks)
    where = sorted({k for k in (0, 767, 768, chunks - 1) if k < chunks} | ({k for k in (3071, 3072) if k < chunks} if chunks > 1536 else set()))
    for k in where:
        part = torch.zeros(chunks, 2, C)
        part[k, 0] = torch.arange(C).float() * 7 + 12345
        part[k, 1] = (1 << 20) - torch.arange(C).float()
        ref = R.bn_finalize(part[k, 0], part[k, 1], n, EPS)
        mean, invstd, _, _ = run_stats(L, part.cuda(), chunks, n, C)
        assert torch.equal(bits(mean), bits((part[k, 0].double() / n).float())), f"row {k} of {chunks} not counted exactly once"
        assert int(R.ulp_distance(invstd, ref["invstd"]).max()) <= 1, f"row {k} of {chunks}: invstd"


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("chunks", CHUNKS)
def test_sync_fwd_sums_from_partials(L, chunks, C):
    """the fp64 sums and n are exact, and zsg_bn_sync_fwd_finalize gives the bits of zsg_bn_stats_from_partials (include/zsg.h's promise)"""
    part, se, sse = partials(chunks, C)
    n = n_for(chunks)
    pd = part.cuda()
    sums = fresh(2 * C + 1, torch.float64)
    L.check(L.lib.zsg_bn_sync_fwd_sums(None, n, C, pd.data_ptr(), chunks, sums.data_ptr(), None, 0, L.stream_ptr()), "bn_sync_fwd_sums")
    got = taken(sums, 2 * C + 1)
    assert torch.equal(got[:C], se) and torch.equal(got[C:2 * C], sse) and float(got[2 * C]) == n
    g = torch.Generator().manual_seed(chunks + C)
    rm0, rv0 = torch.randn(C, generator=g) * 100, torch.rand(C, generator=g) * 1e5 + 1
    mean, invstd, rm, rv = fresh(C), fresh(C), preload(rm0), preload(rv0)
    L.check(L.lib.zsg_bn_sync_fwd_finalize(sums.data_ptr(), C, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), MOM, EPS,
                                           L.stream_ptr()), "bn_sync_fwd_finalize")
    m0, i0, rm1, rv1 = run_stats(L, pd, chunks, n, C, rm0, rv0)
    for a, b, what in ((taken(mean, C), m0, "mean"), (taken(invstd, C), i0, "invstd"), (taken(rm, C), rm1, "running_mean"),
                       (taken(rv, C), rv1, "running_var")):
        assert torch.equal(bits(a), bits(b)), f"{what}: the split finalize differs from zsg_bn_stats_from_partials"


def f32_sum_ref(exact64, pre):
    """dgamma / dbeta as the kernels form them: the fp64 sum rounded to fp32 once, then (accumulate) one fp32 addition to what was there"""
    v = exact64.float()
    return v if pre is None else pre + v


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("chunks", CHUNKS)
def test_backward_from_partials(L, chunks, C):
    """bn_bwd_finalize_kernel on the partial rows, then the apply pass on a small unrelated x / dout (rows = 64; the ABI does not tie
    the partial rows to them).  dbeta = f32(se) and dgamma = f32(sse) exactly (se < 2^24 is an integer fp32 holds; sse is the correctly
    rounded fp32 of the exact fp64 sum), accumulate 0 and 1; coef = f32(se / rows), f32(sse / rows) bit for bit; dx is
    gamma * invstd * (g - c1 - xhat * c2) evaluated in fp32 from those coefficients, to 1e-6 of the expression's terms
    |gamma * invstd| * (|g| + |c1| + |xhat * c2|): seven fp32 roundings of 2^-24 on either side, FMA contraction included."""
    part, se, sse = partials(chunks, C)
    rows = 64
    g = torch.Generator().manual_seed(chunks * 3 + C)
    x, dout = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    mean, invstd, gamma = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    pre_g, pre_b = (torch.randint(-1000, 1001, (C,), generator=g).float() for _ in range(2))
    pd, xd, dd, md, isd, gd = (t.cuda() for t in (part, x, dout, mean, invstd, gamma))
    c1, c2 = (se / rows).float(), (sse / rows).float()
    xh = (x - mean) * invstd
    sc = invstd * gamma
    want_dx = sc * (dout - c1 - xh * c2)
    tol = 1e-6 * (sc.abs() * (dout.abs() + c1.abs() + (xh * c2).abs())).double()
    for acc in (0, 1):
        dx, ws = fresh(rows * C), fresh(2 * C)
        dg, db = (preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))
        L.check(L.lib.zsg_bn_backward_from_partials(dd.data_ptr(), None, xd.data_ptr(), rows, C, md.data_ptr(), isd.data_ptr(), gd.data_ptr(),
                                                    dx.data_ptr(), None, dg.data_ptr(), db.data_ptr(), acc, pd.data_ptr(), chunks,
                                                    ws.data_ptr(), 2 * C * 4, L.stream_ptr()), "bn_backward_from_partials")
        coef = taken(ws, 2 * C)
        assert torch.equal(bits(coef[:C]), bits(c1)) and torch.equal(bits(coef[C:]), bits(c2)), f"coef, accumulate={acc}"
        assert torch.equal(bits(taken(db, C)), bits(f32_sum_ref(se, pre_b if acc else None))), f"dbeta, accumulate={acc}"
        assert torch.equal(bits(taken(dg, C)), bits(f32_sum_ref(sse, pre_g if acc else None))), f"dgamma, accumulate={acc}"
        err = (taken(dx, rows * C).view(rows, C).double() - want_dx.double()).abs()
        assert bool((err <= tol).all()), f"dx: worst error / allowance {float((err / tol).max()):.3g}"


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("chunks", CHUNKS)
def test_sync_bwd_sums_from_partials(L, chunks, C):
    """the fp64 sums exact (no row count travels with the backward sums: the slot after them stays untouched), dgamma / dbeta as above"""
    part, se, sse = partials(chunks, C)
    g = torch.Generator().manual_seed(chunks * 5 + C)
    pre_g, pre_b = (torch.randint(-1000, 1001, (C,), generator=g).float() for _ in range(2))
    pd = part.cuda()
    for acc in (0, 1):
        sums = fresh(2 * C, torch.float64)
        dg, db = (preload(pre_g), preload(pre_b)) if acc else (fresh(C), fresh(C))
        L.check(L.lib.zsg_bn_sync_bwd_sums(None, None, None, 64, C, None, None, pd.data_ptr(), chunks, sums.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                           acc, None, 0, L.stream_ptr()), "bn_sync_bwd_sums")
        got = taken(sums, 2 * C)
        assert torch.equal(got[:C], se) and torch.equal(got[C:], sse), f"sums, accumulate={acc}"
        assert torch.equal(bits(taken(db, C)), bits(f32_sum_ref(se, pre_b if acc else None))), f"dbeta, accumulate={acc}"
        assert torch.equal(bits(taken(dg, C)), bits(f32_sum_ref(sse, pre_g if acc else None))), f"dgamma, accumulate={acc}"


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("which", ["one", "max_minus_1", "max"])
def test_apply_from_partials(L, which, C):
    """the inline reduction of bn_apply_inl_kernel at 1, max - 1 and max = zsg_bn_inline_max_chunks() partial rows: it sums in another
    order than the finalize kernels, which integer rows make irrelevant; max + 1 rows are refused"""
    mx = int(L.lib.zsg_bn_inline_max_chunks())
    chunks = {"one": 1, "max_minus_1": mx - 1, "max": mx}[which]
    part, se, sse = partials(chunks, C)
    rows = n_for(max(chunks, 64))
    g = torch.Generator().manual_seed(chunks * 7 + C)
    x = torch.randn(rows, C, generator=g) * 30
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g) * 100, torch.rand(C, generator=g) * 1e5 + 1
    ref = R.bn_finalize(se, sse, rows, EPS, rm0, rv0, MOM)
    pd, xd, gd, bd = (t.cuda() for t in (part, x, gamma, beta))
    out, mean, invstd, rm, rv = fresh(rows * C), fresh(C), fresh(C), preload(rm0), preload(rv0)
    L.check(L.lib.zsg_bn_apply_from_partials(xd.data_ptr(), rows, C, pd.data_ptr(), chunks, gd.data_ptr(), bd.data_ptr(), None, 0, out.data_ptr(),
                                             None, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), MOM, EPS, L.stream_ptr()),
            "bn_apply_from_partials")
    got_mean, got_invstd = taken(mean, C), taken(invstd, C)
    check_stats(got_mean, got_invstd, taken(rm, C), taken(rv, C), ref, f"chunks={chunks}")
    # out = (x - mean) * (invstd * gamma) + beta in fp32 from the kernel's own statistics: four roundings, 1e-6 of the two terms
    sc = got_invstd * gamma
    want = (x - got_mean) * sc + beta
    err = (taken(out, rows * C).view(rows, C).double() - want.double()).abs()
    assert bool((err <= 1e-6 * (((x - got_mean) * sc).abs() + beta.abs()).double()).all()), f"out off by {float(err.max()):.3g}"


def test_apply_from_partials_refuses_too_many_rows(L):
    mx = int(L.lib.zsg_bn_inline_max_chunks())
    C, rows = 4, 64
    t = torch.zeros((mx + 1) * 2 * C + rows * C, device="cuda")
    s = torch.ones(C, device="cuda")
    rc = L.lib.zsg_bn_apply_from_partials(t.data_ptr(), rows, C, t.data_ptr(), mx + 1, s.data_ptr(), s.data_ptr(), None, 0, t.data_ptr(), None,
                                          s.data_ptr(), s.data_ptr(), None, None, MOM, EPS, L.stream_ptr())
    assert rc == -1 and b"bn_apply_from_partials" in L.lib.zsg_last_error()
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0 and float(s.sum()) == C


def test_bn_stats_conditioning(L, capsys):
    """A characterisation with a DERIVED bound, not a calibrated one: zsg_bn_stats forms var = E[x^2] - m^2 from fp32 per-chunk partial
    sums, so its error grows with (mean / std)^2.  With k fp32 roundings on the longest path of a partial, |delta var| <= 3 k 2^-24 E[x^2];
    for rows = 4096, C = 64 the geometry gives k = 4 + 16 + 1 and the bound takes k = 64 as the cap:
        |invstd / ref - 1| <= 1.5 * 64 * 2^-24 * (1 + ratio^2),   ratio = mean / std in {0, 8, 64}, std = 1,
    against fp64 statistics of the same fp32 data.  The bound is coarse (5.7e-6 at ratio 0, 2.3e-2 at ratio 64) and will not catch every
    regression; the measured maxima it prints, recorded in profiles/bn_stats_conditioning.txt beside torch CPU fp32's, are the point."""
    rows, C = 4096, 64
    x, ratio, inv64 = R.conditioning_data(rows=rows, C=C)
    xd = x.cuda()
    wsb = int(L.lib.zsg_bn_workspace_bytes(rows, C))
    ws = torch.empty(wsb // 4 + 16, device="cuda")
    mean, invstd = fresh(C), fresh(C)
    L.check(L.lib.zsg_bn_stats(xd.data_ptr(), rows, C, mean.data_ptr(), invstd.data_ptr(), None, None, MOM, EPS, ws.data_ptr(), wsb,
                               L.stream_ptr()), "bn_stats")
    err = (taken(invstd, C).double() / inv64 - 1).abs()
    merr = (taken(mean, C).double() - x.double().mean(0)).abs()
    with capsys.disabled():
        for r in (0.0, 8.0, 64.0):
            print(f"\nzsg_bn_stats rows={rows} C={C}, mean/std = {r:g}: max |invstd / fp64 - 1| = {float(err[ratio == r].max()):.3e}, "
                  f"max |mean - fp64| = {float(merr[ratio == r].max()):.3e}", end="")
        print()
    assert bool((err <= 1.5 * 64 * 2.0 ** -24 * (1 + ratio.double() ** 2)).all())

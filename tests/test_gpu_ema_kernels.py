"""zsg_ema_update / zsg_adam_step_ema / zsg_swap_f32 (csrc/ema.hip, csrc/adam.hip) at the C ABI, on seeded data: the update against the fp64
recurrence of tests/ema_ref.py within its bound (every element), the exact cases of the rule (w = 1 a bit copy, w = 0 unchanged bits, NaN
propagation), run-to-run bits, argument errors that write nothing, the fused Adam step against the step followed by a separate update
(bit-equal), and the exchange.  Every buffer sits inside a larger one whose guard elements hold a NaN with a payload: a write outside the
range would change it."""
import pytest
import torch

import ema_ref

pytestmark = pytest.mark.gpu

LENS = [1, 3, 4, 16383, 16385, 3 * (1 << 20) + 5]
NAN_BITS = 0x7FC0BEEF
GUARD = 8          # floats on either side: the payload keeps the 16-byte alignment of the range


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


def guarded(x):
    """x (CPU fp32) on the GPU between two NaN guards -> (whole buffer, the view of x)"""
    g = torch.full((GUARD,), NAN_BITS, dtype=torch.int32).view(torch.float32)
    whole = torch.cat([g, x, g]).cuda()
    return whole, whole[GUARD:GUARD + x.numel()]


def guards_intact(whole):
    w = whole.view(torch.int32)
    return bool((w[:GUARD] == NAN_BITS).all()) and bool((w[-GUARD:] == NAN_BITS).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rand(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def ema_update(L, ea, a, eb=None, b=None, w=0.1):
    two = eb is not None
    return L.lib.zsg_ema_update(ea.data_ptr(), a.data_ptr(), a.numel(), eb.data_ptr() if two else None, b.data_ptr() if two else None,
                                b.numel() if two else 0, w, L.stream_ptr())


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("decay", [0.999, 0.5])
def test_one_range_against_reference(L, n, decay):
    e0, p = rand(n, 1 + n % 97), rand(n, 2 + n % 89, scale=3.0)
    w = ema_ref.weight(decay, False, 1)
    we, e = guarded(e0)
    wp, pp = guarded(p)
    assert ema_update(L, e, pp, w=w) == 0
    torch.cuda.synchronize()
    ema_ref.assert_within(e, ema_ref.step64(e0, p, w), ema_ref.bound1(e0, p), f"n {n} decay {decay}")
    assert guards_intact(we) and guards_intact(wp) and torch.equal(bits(pp), bits(p))


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 4), (4, 3), (16383, 16385), (16385, 1), (5, 1 << 20), (3 * (1 << 20) + 5, 2 * 4803 + 2)])
def test_two_ranges_against_reference_and_single_range_bits(L, na, nb):
    a0, pa, b0, pb = rand(na, 3), rand(na, 4), rand(nb, 5), rand(nb, 6, scale=0.01)
    w = ema_ref.weight(0.9998, False, 1)
    wa, ea = guarded(a0)
    wb, eb = guarded(b0)
    ga, gb = pa.cuda(), pb.cuda()
    assert ema_update(L, ea, ga, eb, gb, w=w) == 0
    torch.cuda.synchronize()
    ema_ref.assert_within(ea, ema_ref.step64(a0, pa, w), ema_ref.bound1(a0, pa), f"range a ({na})")
    ema_ref.assert_within(eb, ema_ref.step64(b0, pb, w), ema_ref.bound1(b0, pb), f"range b ({nb})")
    assert guards_intact(wa) and guards_intact(wb)
    # the same rule on every path: two one-range launches give the two-range launch's bits, and so does a second run
    for src, p, got in ((a0, ga, ea), (b0, gb, eb)):
        for _ in range(2):
            e = src.cuda()
            assert ema_update(L, e, p, w=w) == 0
            assert torch.equal(bits(e), bits(got))


@pytest.mark.parametrize("n", LENS)
def test_exact_cases_copy_unchanged_and_nan(L, n):
    e0, p = rand(n, 7), rand(n, 8, scale=1e-6)          # (tiny p beside O(1) ema: fl(p - e) + e does not round back to p)
    e = e0.cuda()
    assert ema_update(L, e, p.cuda(), w=1.0) == 0
    assert torch.equal(bits(e), bits(p)), "w = 1 is not a bit copy"
    e = e0.cuda()
    assert ema_update(L, e, p.cuda(), w=0.0) == 0
    assert torch.equal(bits(e), bits(e0)), "w = 0 changed the average"
    # NaN / inf in p propagate into exactly their elements, as torch.lerp does; at w = 1 they are copied
    bad = p.clone()
    bad[0] = float("nan")
    bad[n // 2] = float("inf")
    bad[n - 1] = float("-inf") if n > 2 else bad[n - 1]
    e = e0.cuda()
    assert ema_update(L, e, bad.cuda(), w=1.0) == 0
    assert torch.equal(bits(e), bits(bad))
    e = e0.cuda()
    assert ema_update(L, e, bad.cuda(), w=0.25) == 0
    want, got = torch.lerp(e0, bad, 0.25), e.cpu()
    assert not bool(torch.isfinite(want).all())
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
    fin = torch.isfinite(want)
    if bool(fin.any()):
        ema_ref.assert_within(got[fin], ema_ref.step64(e0, bad, 0.25)[fin], ema_ref.bound1(e0, bad)[fin], "finite elements")
    # a NaN average stays NaN below w = 1
    en = e0.clone()
    en[n - 1] = float("nan")
    e = en.cuda()
    assert ema_update(L, e, p.cuda(), w=0.5) == 0
    assert bool(torch.isnan(e[n - 1])) and int(torch.isnan(e).sum()) == 1


def test_argument_errors_return_minus_one_and_write_nothing(L):
    n = 1027
    e0, p = rand(n, 9), rand(n, 10)
    we, e = guarded(e0)
    pp = p.cuda()
    S = L.stream_ptr()
    lib = L.lib
    calls = [
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), n, None, None, 0, 1.5, S),
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), n, None, None, 0, -0.01, S),
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), n, None, None, 0, float("nan"), S),
        lambda: lib.zsg_ema_update(None, pp.data_ptr(), n, None, None, 0, 0.5, S),
        lambda: lib.zsg_ema_update(e.data_ptr(), None, n, None, None, 0, 0.5, S),
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), 0, None, None, 0, 0.5, S),
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), n, e.data_ptr(), None, 4, 0.5, S),          # half a second range
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), n, None, None, 4, 0.5, S),
        lambda: lib.zsg_ema_update(e.data_ptr() + 4, pp.data_ptr(), n - 1, None, None, 0, 0.5, S),            # misaligned
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr() + 8, n - 2, None, None, 0, 0.5, S),
        lambda: lib.zsg_ema_update(e.data_ptr(), pp.data_ptr(), n, e.data_ptr() + 4, pp.data_ptr(), 4, 0.5, S),
        lambda: lib.zsg_swap_f32(e.data_ptr(), pp.data_ptr() + 4, n - 1, S),
        lambda: lib.zsg_swap_f32(None, pp.data_ptr(), n, S),
        lambda: lib.zsg_swap_f32(e.data_ptr(), pp.data_ptr(), 0, S),
        lambda: lib.zsg_swap_f32(e.data_ptr(), e.data_ptr(), n, S),                                           # overlapping: the same range
        lambda: lib.zsg_swap_f32(e.data_ptr(), e.data_ptr() + 16, n - 4, S),                                  # ... shifted by 4 elements
        lambda: lib.zsg_swap_f32(e.data_ptr() + 16 * 100, e.data_ptr(), 401, S),                              # ... by one element at the end
    ]
    for i, c in enumerate(calls):
        assert c() == -1, f"call {i} was accepted"
        assert lib.zsg_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(e), bits(e0)) and torch.equal(bits(pp), bits(p)) and guards_intact(we)
    # adjacent ranges do not overlap
    assert lib.zsg_swap_f32(e.data_ptr(), e.data_ptr() + 16 * 100, 400, S) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(e[:400]), bits(e0[400:800])) and torch.equal(bits(e[400:800]), bits(e0[:400]))
    assert torch.equal(bits(e[800:]), bits(e0[800:])) and guards_intact(we)


@pytest.mark.parametrize("n", LENS)
def test_swap_exchanges_bits_and_twice_is_the_identity(L, n):
    a0, b0 = rand(n, 11), rand(n, 12)
    a0[0] = torch.tensor([NAN_BITS + 1], dtype=torch.int32).view(torch.float32)          # payloads travel too: bits, not values
    wa, a = guarded(a0)
    wb, b = guarded(b0)
    assert L.lib.zsg_swap_f32(a.data_ptr(), b.data_ptr(), n, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b0)) and torch.equal(bits(b), bits(a0))
    assert L.lib.zsg_swap_f32(a.data_ptr(), b.data_ptr(), n, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(b), bits(b0))
    assert guards_intact(wa) and guards_intact(wb)


@pytest.mark.parametrize("n", [1, 3, 4, 16383, 16385, (1 << 21) + 7])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_step_equals_step_then_update(L, n, wd):
    lib, S = L.lib, L.stream_ptr()
    hp = (1e-3, 0.9, 0.99, 1e-8, wd, 0.5)
    p0, e0 = rand(n, 13), rand(n, 14)

    def state():
        wp, p = guarded(p0)
        we, e = guarded(e0)
        return dict(wp=wp, p=p, we=we, e=e, m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"),
                    cnt=torch.zeros(2, dtype=torch.int32, device="cuda"))
    A, B = state(), state()
    for it in range(3):
        g = rand(n, 20 + it, scale=0.1).cuda()
        w = ema_ref.weight(0.9, True, it + 1)
        assert lib.zsg_adam_step_ema(A["p"].data_ptr(), g.data_ptr(), A["m"].data_ptr(), A["v"].data_ptr(), n, *hp, A["cnt"].data_ptr(),
                                     A["e"].data_ptr(), w, S) == 0
        assert lib.zsg_adam_step(B["p"].data_ptr(), g.data_ptr(), B["m"].data_ptr(), B["v"].data_ptr(), n, *hp, B["cnt"].data_ptr(), S) == 0
        assert ema_update(L, B["e"], B["p"], w=w) == 0
        torch.cuda.synchronize()
        for k in ("p", "m", "v", "cnt", "e"):
            assert torch.equal(bits(A[k]), bits(B[k])), f"step {it}: {k} differs between the fused and the separate path"
        assert A["cnt"].tolist() == [it + 1, 0]
    assert not torch.equal(bits(A["p"]), bits(p0)) and not torch.equal(bits(A["e"]), bits(e0))
    assert guards_intact(A["wp"]) and guards_intact(A["we"])
    # the fused entry point's own argument checks: nothing is launched, nothing moves
    before = {k: A[k].clone() for k in ("p", "m", "v", "cnt", "e")}
    g = rand(n, 30).cuda()
    args = lambda e, w: (A["p"].data_ptr(), g.data_ptr(), A["m"].data_ptr(), A["v"].data_ptr(), n, *hp, A["cnt"].data_ptr(), e, w, S)  # noqa: E731
    assert lib.zsg_adam_step_ema(*args(None, 0.5)) == -1
    assert lib.zsg_adam_step_ema(*args(A["e"].data_ptr(), 1.25)) == -1
    assert lib.zsg_adam_step_ema(*args(A["e"].data_ptr(), float("nan"))) == -1
    assert lib.zsg_adam_step_ema(*args(A["e"].data_ptr() + 4, 0.5)) == -1
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(bits(A[k]), bits(t)), k

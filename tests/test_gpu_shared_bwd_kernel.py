"""zsg_head_shared_conv0_bwd through the C ABI: the backward of the sharing point of the shared-image training plan,
    dY[i][p][n] = sum over q ascending with img_idx[q] == i of dy[q][p][n]      (all pyramid levels, packed level-major),
against the host loop `for q: out[idx[q]] += dy[q]` in fp32.  The kernel adds in that very order with plain fp32 adds, so the
comparison is bit for bit (torch.equal), not a tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 256
SIZES_300 = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3)]
CANARY = 1024


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as L
    return L


def host_loop(dys, idx, Bi):
    """fp32, level by level: out[idx[q]] += dy[q] for q ascending; an index outside [0, Bi) contributes nowhere"""
    outs = []
    for dy in dys:
        out = torch.zeros((Bi,) + tuple(dy.shape[1:]), dtype=torch.float32)
        for q in range(dy.shape[0]):
            i = int(idx[q])
            if 0 <= i < Bi:
                out[i] += dy[q]
        outs.append(out)
    return outs


def launch(L, dyd, idd, i64, Bi, Q, sizes, fill=float("nan")):
    """one launch into a dY pre-filled with `fill`, canaries in front of and behind it; returns (dY, canaries intact)"""
    P = sum(h * w for h, w in sizes)
    hw = torch.tensor([v for s_ in sizes for v in s_], dtype=torch.int32)
    buf = torch.full((2 * CANARY + Bi * P * N,), fill, device="cuda")
    buf[:CANARY] = 12345.0
    buf[-CANARY:] = 12345.0
    out = buf[CANARY:CANARY + Bi * P * N]
    L.check(L.lib.zsg_head_shared_conv0_bwd(dyd.data_ptr(), idd.data_ptr(), i64, Bi, Q, len(sizes), hw.data_ptr(), N, out.data_ptr(), L.stream_ptr()),
            "shared conv0 bwd")
    torch.cuda.synchronize()
    ok = bool((buf[:CANARY] == 12345.0).all()) and bool((buf[-CANARY:] == 12345.0).all())
    return out.clone().cpu(), ok


def make_idx(Q, Bi, g, unused=None):
    live = [i for i in range(Bi) if i != unused]
    idx = torch.cat([torch.tensor(live), torch.tensor(live)[torch.randint(0, len(live), (Q - len(live),), generator=g)]]) if Q >= len(live) \
        else torch.tensor(live[:Q])
    return idx[torch.randperm(Q, generator=g)].long()


def unpack(flat, B, sizes):
    out, p0 = [], 0
    for h, w in sizes:
        out.append(flat[B * p0 * N:B * (p0 + h * w) * N].view(B, h, w, N))
        p0 += h * w
    return out


@pytest.mark.parametrize("sizes", [[(5, 5)], SIZES_300], ids=["1level", "5levels"])
@pytest.mark.parametrize("Q,Bi,unused", [(1, 1, None), (6, 1, None), (6, 3, None), (5, 5, None), (16, 4, None), (16, 16, None), (8, 4, 2), (7, 3, 0)],
                         ids=["q1b1", "q6b1", "q6b3", "q5b5", "q16b4", "q16b16", "q8b4_unused2", "q7b3_unused0"])
def test_segmented_sum_is_bit_equal_to_the_host_loop(L, sizes, Q, Bi, unused):
    g = torch.Generator().manual_seed(1000 * Q + 10 * Bi + len(sizes))
    idx = make_idx(Q, Bi, g, unused)
    if unused is None:
        assert sorted(set(idx.tolist())) == list(range(Bi))
    else:
        assert unused not in idx.tolist()
    dys = [torch.randn(Q, h, w, N, generator=g) for h, w in sizes]
    dyd = torch.cat([d.reshape(-1) for d in dys]).cuda()
    ref = host_loop(dys, idx, Bi)
    for i64 in (1, 0):
        idd = idx.cuda() if i64 else idx.int().cuda()
        got, ok = launch(L, dyd, idd, i64, Bi, Q, sizes)                 # dY pre-filled with NaN: every element must be written
        got2, ok2 = launch(L, dyd, idd, i64, Bi, Q, sizes, fill=7.0)
        assert ok and ok2, "a canary around dY was overwritten"
        assert torch.equal(got, got2), "two runs must be bit-identical (and independent of what dY held)"
        for (h, w), r, o in zip(sizes, ref, unpack(got, Bi, sizes)):
            assert torch.equal(o, r), f"level {h}x{w} Q={Q} Bi={Bi} int64={i64}: max |diff| {float((o - r).abs().max()):.3e}"
            if unused is not None:
                assert bool((o[unused] == 0).all()), "an image slot no query points to must get zeros"


@pytest.mark.parametrize("i64", [1, 0], ids=["int64", "int32"])
def test_out_of_range_index_contributes_nowhere_and_touches_nothing_outside(L, i64):
    sizes, Q, Bi = [(5, 5), (3, 3)], 5, 2
    g = torch.Generator().manual_seed(9)
    dys = [torch.randn(Q, h, w, N, generator=g) for h, w in sizes]
    idx = torch.tensor([1, 7, -1, 0, 2], dtype=torch.long)
    # dy sits between canaries too: an out-of-range index must not make the kernel read (let alone write) around it
    P = sum(h * w for h, w in sizes)
    src = torch.full((2 * CANARY + Q * P * N,), float("nan"), device="cuda")
    src[CANARY:CANARY + Q * P * N] = torch.cat([d.reshape(-1) for d in dys]).cuda()
    dyd = src[CANARY:CANARY + Q * P * N]
    idd = idx.cuda() if i64 else idx.int().cuda()
    got, ok = launch(L, dyd, idd, i64, Bi, Q, sizes)
    assert ok, "a canary around dY was overwritten"
    assert torch.isnan(src[:CANARY]).all() and torch.isnan(src[-CANARY:]).all()
    assert torch.isfinite(got).all(), "something outside dy (NaN) was read"
    for r, o in zip(host_loop(dys, idx, Bi), unpack(got, Bi, sizes)):
        assert torch.equal(o, r)


def test_bad_arguments_are_refused(L):
    d = torch.zeros(9 * N, device="cuda")
    i = torch.zeros(1, dtype=torch.long, device="cuda")
    hw = torch.tensor([3, 3], dtype=torch.int32)
    st = L.stream_ptr()
    assert L.lib.zsg_head_shared_conv0_bwd(d.data_ptr(), i.data_ptr(), 1, 0, 1, 1, hw.data_ptr(), N, d.data_ptr(), st) != 0          # Bi == 0
    assert L.lib.zsg_head_shared_conv0_bwd(d.data_ptr(), i.data_ptr(), 1, 1, 1, 1, hw.data_ptr(), 6, d.data_ptr(), st) != 0          # N % 4
    assert L.lib.zsg_head_shared_conv0_bwd(None, i.data_ptr(), 1, 1, 1, 1, hw.data_ptr(), N, d.data_ptr(), st) != 0

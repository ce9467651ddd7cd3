"""zsg_adam_step_segments (csrc/adam.hip) at the C ABI: Adam over listed segments of a flat buffer with per-group hyperparameters and
per-segment step counters, against torch.optim.Adam on per-segment tensors; the elements between segments are never touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


def seg_table(L, segs):
    """segs: [(off, len, group, counter)] -> (device table, nseg, nchunks)"""
    arr = (L.AdamSeg * len(segs))()
    chunk = 0
    for k, (off, n, gi, ci) in enumerate(segs):
        arr[k] = L.AdamSeg(off, n, gi, ci, chunk, 0)
        chunk += (n + L.ADAM_CHUNK - 1) // L.ADAM_CHUNK
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return tab, len(segs), chunk


def groups_of(L, hps):
    return (L.AdamGroup * len(hps))(*[L.AdamGroup(*h) for h in hps])


NAN_BITS = 0x7FC0BEEF          # a quiet NaN with a payload: any write of a computed value changes it


def test_segments_match_torch_and_leave_gaps_alone(L):
    g = torch.Generator().manual_seed(3)
    # (length, group): odd lengths, one spanning several work chunks, one shorter than a vector
    lens = [(7, 0), (4099, 1), (2 * L.ADAM_CHUNK + 5, 2), (1, 0), (33, 1), (520, 2)]
    late = 4                                    # this segment joins at step 2 (its parameter was frozen before): bias correction from t = 1
    hps = [(1e-2, 0.9, 0.99, 1e-8, 0.0), (3e-3, 0.8, 0.999, 1e-6, 0.05), (5e-4, 0.95, 0.9, 1e-7, 0.0)]
    segs, off = [], 4                           # a gap in front of the first segment too
    for k, (n, gi) in enumerate(lens):
        segs.append((off, n, gi, k))
        off += (n + 3) // 4 * 4 + 4 * (1 + k % 3)          # gaps of 4..12 elements behind every segment
    total = off + 8
    gap = torch.ones(total, dtype=torch.bool)
    for (o, n, _, _) in segs:
        gap[o:o + n] = False
    nanv = torch.tensor([NAN_BITS], dtype=torch.int32).view(torch.float32)

    def fresh(x):
        t = torch.where(gap, nanv.expand(total), x)
        return t.cuda()
    p = fresh(torch.randn(total, generator=g))
    m, v = fresh(torch.zeros(total)), fresh(torch.zeros(total))
    gd = torch.full((total,), float("nan"), device="cuda")
    p_gap, m_gap, v_gap = (t[gap.cuda()].view(torch.int32).clone() for t in (p, m, v))
    tps = [torch.nn.Parameter(p[o:o + n].detach().cpu().clone()) for (o, n, _, _) in segs]
    topt = torch.optim.Adam([dict(params=[tp for tp, s in zip(tps, segs) if s[2] == gi], lr=h[0], betas=(h[1], h[2]), eps=h[3],
                                  weight_decay=h[4]) for gi, h in enumerate(hps)])
    counters = torch.zeros(len(segs), dtype=torch.int32, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    gt = groups_of(L, hps)
    for it in range(5):
        on = [k for k in range(len(segs)) if k != late or it >= 2]
        tab, nseg, nch = seg_table(L, [segs[k] for k in on])
        for k, (o, n, _, _) in enumerate(segs):
            gr = torch.randn(n, generator=g)
            gd[o:o + n] = gr.cuda()
            tps[k].grad = gr.clone() if k in on else None          # torch's rule: no gradient, no step
        topt.step()
        L.check(L.lib.zsg_adam_step_segments(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), tab.data_ptr(), nseg, nch, gt, len(hps),
                                             1.0, counters.data_ptr(), ticket.data_ptr(), L.stream_ptr()), "adam segments")
    torch.cuda.synchronize()
    assert counters.tolist() == [5 if k != late else 3 for k in range(len(segs))] and int(ticket) == 0
    for t, ref in ((p, p_gap), (m, m_gap), (v, v_gap)):
        assert torch.equal(t[gap.cuda()].view(torch.int32), ref), "an element outside the listed segments was written"
    for k, (o, n, _, _) in enumerate(segs):
        torch.testing.assert_close(p[o:o + n].cpu(), tps[k].detach(), rtol=1e-5, atol=1e-6, msg=f"segment {k}")
        # (the moments carry (1 - beta) rounded through the fp32 beta, as zsg_adam_step does: 1 - 0.999f is 1.3e-5 off 0.001)
        st = topt.state[tps[k]]
        torch.testing.assert_close(m[o:o + n].cpu(), st["exp_avg"], rtol=1e-4, atol=1e-7)
        torch.testing.assert_close(v[o:o + n].cpu(), st["exp_avg_sq"], rtol=1e-4, atol=1e-9)


def test_one_segment_one_group_is_the_flat_step_bit_for_bit(L):
    g = torch.Generator().manual_seed(5)
    n = 3 * L.ADAM_CHUNK + 4099
    p0 = torch.randn(n, generator=g).cuda()
    pa, pb = p0.clone(), p0.clone()
    ma, mb, va, vb = (torch.zeros(n, device="cuda") for _ in range(4))
    step2 = torch.zeros(2, dtype=torch.int32, device="cuda")
    counters, ticket = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    tab, nseg, nch = seg_table(L, [(0, n, 0, 0)])
    hp = (2e-3, 0.9, 0.99, 1e-8, 1e-2)
    gt = groups_of(L, [hp])
    for it in range(4):
        gr = torch.randn(n, generator=g).cuda()
        L.check(L.lib.zsg_adam_step(pa.data_ptr(), gr.data_ptr(), ma.data_ptr(), va.data_ptr(), n, *hp, 0.5, step2.data_ptr(), L.stream_ptr()), "adam")
        L.check(L.lib.zsg_adam_step_segments(pb.data_ptr(), gr.data_ptr(), mb.data_ptr(), vb.data_ptr(), tab.data_ptr(), nseg, nch, gt, 1, 0.5,
                                             counters.data_ptr(), ticket.data_ptr(), L.stream_ptr()), "adam segments")
    torch.cuda.synchronize()
    assert step2.tolist() == [4, 0] and counters.tolist() == [4] and int(ticket) == 0
    for a, b in ((pa, pb), (ma, mb), (va, vb)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_group_limit_is_enforced(L):
    t = torch.zeros(16, device="cuda")
    tab, nseg, nch = seg_table(L, [(0, 16, 0, 0)])
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    gt = groups_of(L, [(1e-3, 0.9, 0.99, 1e-8, 0.0)] * (L.ADAM_MAX_GROUPS + 1))
    rc = L.lib.zsg_adam_step_segments(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), tab.data_ptr(), nseg, nch, gt, L.ADAM_MAX_GROUPS + 1,
                                      1.0, cnt.data_ptr(), cnt[1:].data_ptr(), L.stream_ptr())
    assert rc != 0 and b"parameter groups" in L.lib.zsg_last_error()

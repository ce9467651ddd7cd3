"""zsg_grad_norm / zsg_grad_scale (csrc/clip.hip) at the C ABI: the total 2- / inf-norm of listed segments of a flat buffer, torch's
clip coefficient, and the in-place scale, against numpy fp64 and torch.nn.utils.clip_grad_norm_ on per-segment tensors.  The gaps between
segments hold NaN: an element read outside the listed ranges would turn every norm NaN, and one written would lose its payload."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


NAN_BITS = 0x7FC0BEEF          # a quiet NaN with a payload: any write of a computed value changes it


def seg_table(L, segs):
    """segs: [(off, len)] -> (device table, nseg, nchunks)"""
    arr = (L.AdamSeg * max(1, len(segs)))()
    chunk = 0
    for k, (off, n) in enumerate(segs):
        arr[k] = L.AdamSeg(off, n, 0, k, chunk, 0)
        chunk += (n + L.ADAM_CHUNK - 1) // L.ADAM_CHUNK
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return tab, len(segs), chunk


class Buf:
    """a flat buffer of random segments (odd lengths, a length-1 segment, several multi-chunk ones) with NaN gaps around them"""

    def __init__(self, L, seed=3, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        lens = [7, 1, 4099, 2 * L.ADAM_CHUNK + 5, 33, 3 * L.ADAM_CHUNK, 520, L.ADAM_CHUNK + 1]
        self.segs, off = [], 4
        for k, n in enumerate(lens):
            self.segs.append((off, n))
            off += (n + 3) // 4 * 4 + 4 * (1 + k % 3)          # gaps of 4..12 elements behind every segment
        self.total = off + 8
        self.gap = torch.ones(self.total, dtype=torch.bool)
        for o, n in self.segs:
            self.gap[o:o + n] = False
        x = torch.randn(self.total, generator=g) * scale
        x[self.gap] = torch.tensor([NAN_BITS], dtype=torch.int32).view(torch.float32)
        self.g = x.cuda()
        self.gap = self.gap.cuda()
        self.tab, self.nseg, self.nch = seg_table(L, self.segs)
        self.partials = torch.empty(self.nch, dtype=torch.float64, device="cuda")
        self.ticket = torch.zeros(1, dtype=torch.int32, device="cuda")

    def pieces(self, t=None):
        t = self.g if t is None else t
        return [t[o:o + n] for o, n in self.segs]

    def norm(self, L, inf, max_norm):
        out = torch.full((2,), -7.0, device="cuda")
        L.check(L.lib.zsg_grad_norm(self.g.data_ptr(), self.tab.data_ptr(), self.nseg, self.nch, 1 if inf else 0, max_norm,
                                    self.partials.data_ptr(), self.ticket.data_ptr(), out.data_ptr(), L.stream_ptr()), "grad_norm")
        torch.cuda.synchronize()
        assert int(self.ticket) == 0
        return out

    def scale(self, L, out):
        L.check(L.lib.zsg_grad_scale(self.g.data_ptr(), self.tab.data_ptr(), self.nseg, self.nch, out.data_ptr() + 4, L.stream_ptr()),
                "grad_scale")
        torch.cuda.synchronize()


def torch_coef(tn, max_norm):
    """clip_coef of torch.nn.utils._clip_grads_with_norm_ for an fp32 total norm, on the GPU"""
    return torch.clamp(max_norm / (torch.tensor(tn, dtype=torch.float32, device="cuda") + 1e-6), max=1.0)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("inf", [False, True], ids=["l2", "inf"])
def test_norm_coefficient_and_scale(L, inf):
    b = Buf(L, seed=3 if inf else 4)
    x = np.concatenate([p.cpu().numpy() for p in b.pieces()]).astype(np.float64)
    ref = np.abs(x).max() if inf else math.sqrt(float((x * x).sum()))
    g0 = b.g.clone()
    max_norm = 0.25 * float(ref)                      # engages
    out = b.norm(L, inf, max_norm)
    tn, coef = out.cpu().tolist()
    if inf:
        assert tn == float(np.float32(ref)), "the inf-norm is exact"
    else:
        assert abs(tn - ref) <= 1e-6 * ref, (tn, ref)
    assert bits(out[1:]).item() == bits(torch_coef(tn, max_norm).reshape(1)).item(), (coef, float(torch_coef(tn, max_norm)))
    assert 0 < coef < 1
    b.scale(L, out)
    for p, p0 in zip(b.pieces(), b.pieces(g0)):
        assert torch.equal(bits(p), bits(p0 * out[1])), "scaled range != g * coef"
    assert torch.equal(bits(b.g[b.gap]), bits(g0[b.gap])), "an element outside the listed segments was written"
    # the same gradients against torch's own clip_grad_norm_ on per-segment tensors
    ps = [torch.nn.Parameter(torch.zeros_like(p)) for p in b.pieces(g0)]
    for p, p0 in zip(ps, b.pieces(g0)):
        p.grad = p0.clone()
    tt = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=math.inf if inf else 2.0)
    assert abs(float(tt) - tn) <= 1e-6 * tn
    for p, mine in zip(ps, b.pieces()):
        torch.testing.assert_close(mine, p.grad, rtol=1e-6, atol=0)


@pytest.mark.parametrize("inf", [False, True], ids=["l2", "inf"])
def test_unit_coefficient_leaves_the_buffer_bitwise(L, inf):
    b = Buf(L, seed=5)
    g0 = b.g.clone()
    out = b.norm(L, inf, 1e9)
    assert float(out[1]) == 1.0
    b.scale(L, out)
    assert torch.equal(bits(b.g), bits(g0))


def test_two_calls_are_bit_identical_in_either_reduction_mode(L):
    b = Buf(L, seed=6, scale=1e-3)
    outs = []
    try:
        for det in (0, 1, 0):
            L.lib.zsg_set_deterministic(det)
            outs += [b.norm(L, False, 1e-4).clone(), b.norm(L, True, 1e-4).clone()]
    finally:
        L.lib.zsg_set_deterministic(1 if os.environ.get("ZSG_DETERMINISTIC", "0") == "1" else 0)
    for k in range(2, len(outs)):
        assert torch.equal(bits(outs[k]), bits(outs[k % 2])), k


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("inf", [False, True], ids=["l2", "inf"])
def test_nonfinite_gradients_follow_torch(L, inf, bad):
    b = Buf(L, seed=7)
    o, n = b.segs[3]
    b.g[o + n // 2] = bad
    g0 = b.g.clone()
    ps = [torch.nn.Parameter(torch.zeros_like(p)) for p in b.pieces(g0)]
    for p, p0 in zip(ps, b.pieces(g0)):
        p.grad = p0.clone()
    tt = torch.nn.utils.clip_grad_norm_(ps, 1.0, norm_type=math.inf if inf else 2.0)
    out = b.norm(L, inf, 1.0)
    tn, coef = out.cpu().tolist()
    ttn = float(tt)
    assert (math.isnan(tn) and math.isnan(ttn)) or tn == ttn, (tn, ttn)
    tc = float(torch_coef(ttn, 1.0))
    assert (math.isnan(coef) and math.isnan(tc)) or coef == tc, (coef, tc)
    b.scale(L, out)
    for p, mine in zip(ps, b.pieces()):
        torch.testing.assert_close(mine, p.grad, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(bits(b.g[b.gap]), bits(g0[b.gap]))


def test_zero_segments_launch_nothing(L):
    b = Buf(L, seed=8)
    out = torch.full((2,), -7.0, device="cuda")
    g0 = b.g.clone()
    L.lib.zsg_prof_enable(1)
    try:
        L.lib.zsg_prof_collect((L.ProfEntry * 64)(), 64)          # (drop earlier records)
        L.check(L.lib.zsg_grad_norm(b.g.data_ptr(), b.tab.data_ptr(), 0, 0, 0, 1.0, b.partials.data_ptr(), b.ticket.data_ptr(),
                                    out.data_ptr(), L.stream_ptr()), "grad_norm")
        L.check(L.lib.zsg_grad_scale(b.g.data_ptr(), b.tab.data_ptr(), 0, 0, out.data_ptr() + 4, L.stream_ptr()), "grad_scale")
        one, _, _ = seg_table(L, b.segs[:1])
        L.check(L.lib.zsg_grad_norm(b.g.data_ptr(), one.data_ptr(), 1, 1, 0, 1e9, b.partials.data_ptr(), b.ticket.data_ptr(),
                                    out.data_ptr(), L.stream_ptr()), "grad_norm")          # (positive control: one launch)
        torch.cuda.synchronize()
        ents = (L.ProfEntry * 64)()
        n = L.lib.zsg_prof_collect(ents, 64)
    finally:
        L.lib.zsg_prof_enable(0)
    launches = {ents[i].name.decode(): ents[i].launches for i in range(n)}
    assert launches.get("grad_norm") == 1 and "grad_scale" not in launches, launches
    assert torch.equal(bits(b.g), bits(g0))
    o, k = b.segs[0]
    assert float(out[0]) == pytest.approx(float(g0[o:o + k].double().norm()), rel=1e-6)

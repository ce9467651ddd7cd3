"""zsg_lamb_moments / zsg_lamb_apply (csrc/lamb.hip) at the C ABI against tests/lamb_ref.py: three steps over segments of 1, 3, 4, 5,
ZSG_ADAM_CHUNK, ZSG_ADAM_CHUNK + 1 and 2 * ZSG_ADAM_CHUNK + 7 elements in three groups (one of them adapt = 0); a case in which every
operation is exact, compared bit for bit; what one segment may do to another (nothing); run-to-run bit identity; the counters; argument
errors that launch and write nothing.  As tests/test_gpu_optim_kernels.py the buffers carry NaN guards with a payload on either side and
NaN gaps between the segments: a write outside the listed ranges would change them."""
import numpy as np
import pytest
import torch

import lamb_ref

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF          # a quiet NaN with a payload: any write of a computed value changes it
GUARD = 8                      # floats in front of the first and behind the last segment (keeps the 16-byte alignment)
CHUNK = 16384
LENS = [(1, 0), (3, 1), (4, 2), (5, 0), (CHUNK, 1), (CHUNK + 1, 2), (2 * CHUNK + 7, 0)]          # (elements, group)
# three groups: adaptive without decay, NOT adaptive with decay, adaptive with decay
HPS = [dict(lr=1e-2, b1=0.9, b2=0.99, eps=1e-8, wd=0.0, adapt=1), dict(lr=3e-3, b1=0.8, b2=0.999, eps=1e-6, wd=0.05, adapt=0),
       dict(lr=5e-3, b1=0.95, b2=0.9, eps=1e-7, wd=0.01, adapt=1)]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    assert _lib.ADAM_CHUNK == CHUNK
    return _lib


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def group(L, h):
    return L.LambGroup(h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["adapt"])


class Layout:
    """segments (off, len, group, counter) with gaps of 4..12 elements between them and GUARD elements at either end"""

    def __init__(self, lens=LENS):
        self.segs, off = [], GUARD
        for k, (n, gi) in enumerate(lens):
            self.segs.append((off, n, gi, k))
            off += (n + 3) // 4 * 4 + 4 * (1 + k % 3)
        self.total = off - 4 * (1 + (len(lens) - 1) % 3) + GUARD
        self.gap = torch.ones(self.total, dtype=torch.bool)
        for (o, n, _, _) in self.segs:
            self.gap[o:o + n] = False
        self.nanv = torch.tensor([NAN_BITS], dtype=torch.int32).view(torch.float32)

    def fresh(self, x):
        """x inside the segments, the payload NaN everywhere else, on the GPU"""
        return torch.where(self.gap, self.nanv.expand(self.total), x).cuda()

    def table(self, L, on=None):
        on = range(len(self.segs)) if on is None else on
        arr = (L.AdamSeg * len(on))()
        chunk = 0
        for k, s in enumerate(on):
            off, n, gi, ci = self.segs[s]
            arr[k] = L.AdamSeg(off, n, gi, ci, chunk, 0)
            chunk += (n + CHUNK - 1) // CHUNK
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), len(on), chunk


class Run:
    """p, m, v between guards and gaps, counters, ticket, scratch; step() = the two launches"""

    def __init__(self, L, lay, p0, hps=HPS):
        self.L, self.lay, self.hps = L, lay, hps
        self.p = lay.fresh(p0)
        self.m, self.v = lay.fresh(torch.zeros(lay.total)), lay.fresh(torch.zeros(lay.total))
        self.counters = torch.zeros(len(lay.segs), dtype=torch.int32, device="cuda")
        self.ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stats = []          # per step: (ratio, norm_w, norm_u) [3, nseg] of the listed segments

    def step(self, g, on=None, gs=1.0):
        L, lay = self.L, self.lay
        tab, nseg, nch = lay.table(L, on)
        gd = lay.fresh(g)
        part = torch.full((2 * nch,), float("nan"), dtype=torch.float64, device="cuda")
        st = torch.full((3, nseg), float("nan"), device="cuda")
        gt = (L.LambGroup * len(self.hps))(*[group(L, h) for h in self.hps])
        sp = L.stream_ptr()
        L.check(L.lib.zsg_lamb_moments(self.p.data_ptr(), gd.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), tab.data_ptr(), nseg, nch, gt,
                                       len(self.hps), gs, self.counters.data_ptr(), part.data_ptr(), self.ticket.data_ptr(), st[0].data_ptr(),
                                       st[1].data_ptr(), st[2].data_ptr(), sp), "lamb_moments")
        L.check(L.lib.zsg_lamb_apply(self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), tab.data_ptr(), nseg, nch, gt, len(self.hps),
                                     st[0].data_ptr(), self.counters.data_ptr(), self.ticket.data_ptr(), sp), "lamb_apply")
        self.stats.append(st)
        return self

    def all_bits(self):
        torch.cuda.synchronize()
        return [bits(t) for t in (self.p, self.m, self.v)] + [bits(s) for s in self.stats] + [self.counters.cpu(), self.ticket.cpu()]

    def gaps_intact(self):
        gapd = self.lay.gap.cuda()
        return all(bool((t.view(torch.int32)[gapd] == NAN_BITS).all()) for t in (self.p, self.m, self.v))


def inputs(lay, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(lay.total, generator=g), [torch.randn(lay.total, generator=g) for _ in range(steps)]


def reference(lay, p0, grads, hps=HPS, gss=None):
    """lamb_ref over every segment and step -> per segment (w, m, v, [info per step])"""
    out = []
    for (o, n, gi, _) in lay.segs:
        h = hps[gi]
        w, m, v, infos = p0[o:o + n].numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32), []
        for t, g in enumerate(grads):
            w, m, v, info = lamb_ref.lamb_step(w, g[o:o + n].numpy(), m, v, t + 1, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], bool(h["adapt"]),
                                               1.0 if gss is None else gss[t])
            infos.append(info)
        out.append((w, m, v, infos))
    return out


@pytest.fixture(scope="module")
def three_steps(L):
    """one run of three steps (grad_scale = 0.5 on the second) and its reference, shared by the tests below and left unchanged"""
    lay = Layout()
    p0, grads = inputs(lay, 3, seed=3)
    gss = [1.0, 0.5, 1.0]
    run = Run(L, lay, p0)
    for g, gs in zip(grads, gss):
        run.step(g, gs=gs)
    torch.cuda.synchronize()
    return lay, p0, grads, gss, run, reference(lay, p0, grads, gss=gss)


def test_three_steps_match_the_reference(L, three_steps):
    lay, _, _, _, run, ref = three_steps
    assert [n for n, _ in LENS] == [1, 3, 4, 5, CHUNK, CHUNK + 1, 2 * CHUNK + 7] and sorted({gi for _, gi in LENS}) == [0, 1, 2]
    assert run.counters.tolist() == [3] * len(lay.segs) and int(run.ticket) == 0
    assert run.gaps_intact(), "an element outside the listed segments was written"
    p, m, v = run.p.cpu(), run.m.cpu(), run.v.cpu()
    for k, ((o, n, gi, _), (rw, rm, rv, infos)) in enumerate(zip(lay.segs, ref)):
        msg = lambda what: (lambda s, k=k, what=what: f"segment {k} (len {n}) {what}: {s}")          # noqa: E731
        torch.testing.assert_close(m[o:o + n], torch.from_numpy(rm), rtol=1e-4, atol=1e-7, msg=msg("m"))
        torch.testing.assert_close(v[o:o + n], torch.from_numpy(rv), rtol=1e-4, atol=1e-9, msg=msg("v"))
        torch.testing.assert_close(p[o:o + n], torch.from_numpy(rw), rtol=1e-5, atol=1e-6, msg=msg("p"))
        for t, info in enumerate(infos):
            got = run.stats[t][:, k].cpu().tolist()
            want = [float(info["ratio"]), float(info["norm_w"]), float(info["norm_u"])]
            print(f"segment {k} step {t + 1}: ratio, |w|, |u| = {got}, reference {want}")
            for a, b, what in zip(got, want, ("ratio", "norm_w", "norm_u")):
                assert abs(a - b) <= 1e-5 * abs(b), f"segment {k} step {t + 1} {what}: {a} against {b}"
            if not HPS[gi]["adapt"]:
                assert got[0] == 1.0 and want[0] == 1.0


def test_run_to_run_bit_identity(L, three_steps):
    lay, p0, grads, gss, run, _ = three_steps
    again = Run(L, lay, p0)
    for g, gs in zip(grads, gss):
        again.step(g, gs=gs)
    assert all(torch.equal(a, b) for a, b in zip(run.all_bits(), again.all_bits()))


def exact_case():
    """t = 1, beta1 = 1/2, beta2 = 3/4, eps = 0, wd = 0, gradients +-2^k: m = g / 2, v = g^2 / 4, bc1 = 1/2, bc2 = 1/4, u = sign(g).  16
    gradients: |u| = 4.  Weights four 3s, seven 2s and five 0s in mixed signs: sum w^2 = 36 + 28 = 64, |w| = 8, ratio 2; lr = 1/4."""
    ks = [-3, 4, 0, 1, -2, 3, 2, -1, 4, -3, 1, 0, 3, -2, -1, 2]
    sg = [1, -1, -1, 1, 1, 1, -1, -1, 1, -1, 1, 1, -1, -1, 1, -1]
    g = torch.tensor([s * 2.0 ** k for s, k in zip(sg, ks)])
    w = torch.tensor([3.0, -2, 0, 2, -3, 2, 0, -2, 2, 3, 0, -2, 0, 2, -3, 0])
    h = dict(lr=0.25, b1=0.5, b2=0.75, eps=0.0, wd=0.0, adapt=1)
    return w, g, h


def test_the_reference_is_exact_for_the_exact_case():
    w, g, h = exact_case()
    assert int((g != 0).sum()) == 16 and float((w.double() ** 2).sum()) == 64.0
    w1, m1, v1, info = lamb_ref.lamb_step(w.numpy(), g.numpy(), np.zeros(16), np.zeros(16), 1, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"])
    assert np.array_equal(info["u"], np.sign(g.numpy())) and float(info["norm_u"]) == 4.0 and float(info["norm_w"]) == 8.0
    assert float(info["ratio"]) == 2.0 and float(info["norm_w"]) / 4 == 2.0
    assert np.array_equal(m1, g.numpy() / 2) and np.array_equal(v1, g.numpy() ** 2 / 4)
    assert np.array_equal(w1, w.numpy() - 0.5 * np.sign(g.numpy()))


def test_exact_case_is_bit_equal_to_the_reference(L):
    w, g, h = exact_case()
    lay = Layout([(16, 0)])
    p0, g0 = torch.zeros(lay.total), torch.zeros(lay.total)
    o = lay.segs[0][0]
    p0[o:o + 16], g0[o:o + 16] = w, g
    run = Run(L, lay, p0, hps=[h]).step(g0)
    torch.cuda.synchronize()
    w1, m1, v1, info = lamb_ref.lamb_step(w.numpy(), g.numpy(), np.zeros(16), np.zeros(16), 1, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"])
    for got, want, what in ((run.p, w1, "p"), (run.m, m1, "m"), (run.v, v1, "v")):
        assert torch.equal(bits(got[o:o + 16]), bits(torch.from_numpy(want))), what
    assert torch.equal(bits(run.stats[0][:, 0]), bits(torch.tensor([2.0, 8.0, 4.0])))
    assert run.gaps_intact() and run.counters.tolist() == [1] and int(run.ticket) == 0


def test_isolation_of_segments(L):
    lay = Layout()
    p0, (g0,) = inputs(lay, 1, seed=11)
    zero_w, zero_g, hit = 3, 6, 5          # segments of the adaptive groups 0 and 2 (group 0 has no decay)
    assert LENS[zero_w][1] == 0 and LENS[zero_g][1] == 0 and LENS[hit] == (CHUNK + 1, 2) and HPS[0]["wd"] == 0.0 and HPS[0]["adapt"] and HPS[2]["adapt"]
    ow, nw = lay.segs[zero_w][:2]
    og, ng = lay.segs[zero_g][:2]
    oh, nh = lay.segs[hit][:2]
    p0[ow:ow + nw] = 0.0
    g0[og:og + ng] = 0.0
    clean = Run(L, lay, p0).step(g0)
    torch.cuda.synchronize()
    r = clean.stats[0][0].cpu()
    assert float(r[zero_w]) == 1.0 and float(clean.stats[0][1][zero_w]) == 0.0, "w = 0: the ratio is 1"
    assert bool((clean.p[ow:ow + nw] != 0).all()), "... and the segment still takes its Adam step"
    assert float(r[zero_g]) == 1.0 and float(clean.stats[0][2][zero_g]) == 0.0
    assert torch.equal(bits(clean.p[og:og + ng]), bits(p0[og:og + ng])), "g = 0 at t = 1 without decay: p keeps its bits"
    # a NaN gradient in the second chunk of one segment: the whole segment goes NaN (its ratio does), nothing else changes by a bit
    bad = g0.clone()
    bad[oh + CHUNK] = float("nan")
    dirty = Run(L, lay, p0).step(bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dirty.p[oh:oh + nh]).all()) and bool(torch.isnan(dirty.stats[0][0][hit]))
    keep = torch.ones(lay.total, dtype=torch.bool)
    keep[oh:oh + nh] = False
    for a, b, what in zip((clean.p, clean.m, clean.v), (dirty.p, dirty.m, dirty.v), "pmv"):
        assert torch.equal(bits(a)[keep], bits(b)[keep]), f"{what}: another segment, a gap or a guard changed"
    others = [k for k in range(len(lay.segs)) if k != hit]
    assert torch.equal(bits(clean.stats[0][:, others]), bits(dirty.stats[0][:, others]))
    assert dirty.gaps_intact() and dirty.counters.tolist() == [1] * len(lay.segs)


def test_counters_advance_for_listed_segments_only(L):
    lay = Layout()
    p0, grads = inputs(lay, 2, seed=13)
    out = 4
    on = [k for k in range(len(lay.segs)) if k != out]
    run = Run(L, lay, p0).step(grads[0], on=on)
    torch.cuda.synchronize()
    assert run.counters.tolist() == [0 if k == out else 1 for k in range(len(lay.segs))] and int(run.ticket) == 0
    o, n = lay.segs[out][:2]
    assert torch.equal(bits(run.p[o:o + n]), bits(p0[o:o + n])) and not bool(run.m[o:o + n].any()) and not bool(run.v[o:o + n].any())
    # the late segment's first step is its t = 1, beside the others' t = 2
    run.step(grads[1])
    torch.cuda.synchronize()
    assert run.counters.tolist() == [1 if k == out else 2 for k in range(len(lay.segs))] and run.gaps_intact()
    h = HPS[lay.segs[out][2]]
    w1, m1, v1, _ = lamb_ref.lamb_step(p0[o:o + n].numpy(), grads[1][o:o + n].numpy(), np.zeros(n), np.zeros(n), 1, h["lr"], h["b1"], h["b2"],
                                       h["eps"], h["wd"], bool(h["adapt"]))
    torch.testing.assert_close(run.m[o:o + n].cpu(), torch.from_numpy(m1), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(run.v[o:o + n].cpu(), torch.from_numpy(v1), rtol=1e-4, atol=1e-9)
    torch.testing.assert_close(run.p[o:o + n].cpu(), torch.from_numpy(w1), rtol=1e-5, atol=1e-6)


def _launches(L, fn):
    L.lib.zsg_prof_enable(1)
    try:
        L.lib.zsg_prof_collect((L.ProfEntry * 256)(), 256)          # (drop earlier records)
        fn()
        torch.cuda.synchronize()
        ents = (L.ProfEntry * 256)()
        n = L.lib.zsg_prof_collect(ents, 256)
    finally:
        L.lib.zsg_prof_enable(0)
    return {ents[i].name.decode(): (ents[i].launches, ents[i].bytes) for i in range(n)}


def test_two_launches_per_step_and_argument_errors_write_nothing(L):
    lay = Layout()
    p0, (g0,) = inputs(lay, 1, seed=17)
    run = Run(L, lay, p0)
    nch = lay.table(L)[2]
    got = _launches(L, lambda: run.step(g0))
    assert got == {"lamb_moments": (1, 24.0 * nch * CHUNK), "lamb_apply": (1, 16.0 * nch * CHUNK)}, got
    keep = run.all_bits()
    tab, nseg, _ = lay.table(L)
    gd = lay.fresh(g0)
    part = torch.full((2 * nch,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((3, nseg), float("nan"), device="cuda")
    part0, st0 = bits(part.view(torch.float32)), bits(st)
    gt = (L.LambGroup * len(HPS))(*[group(L, h) for h in HPS])
    many = (L.LambGroup * (L.ADAM_MAX_GROUPS + 1))(*[group(L, HPS[0])] * (L.ADAM_MAX_GROUPS + 1))
    base = dict(p=run.p.data_ptr(), g=gd.data_ptr(), m=run.m.data_ptr(), v=run.v.data_ptr(), segs=tab.data_ptr(), nseg=nseg, nchunks=nch, groups=gt,
                ngroups=len(HPS), gs=1.0, counters=run.counters.data_ptr(), partials=part.data_ptr(), ticket=run.ticket.data_ptr(),
                ratio=st[0].data_ptr(), norm_w=st[1].data_ptr(), norm_u=st[2].data_ptr())

    def moments(**kw):
        a = dict(base, **kw)
        return L.lib.zsg_lamb_moments(a["p"], a["g"], a["m"], a["v"], a["segs"], a["nseg"], a["nchunks"], a["groups"], a["ngroups"], a["gs"],
                                      a["counters"], a["partials"], a["ticket"], a["ratio"], a["norm_w"], a["norm_u"], L.stream_ptr())

    def apply(**kw):
        a = dict(base, **kw)
        return L.lib.zsg_lamb_apply(a["p"], a["m"], a["v"], a["segs"], a["nseg"], a["nchunks"], a["groups"], a["ngroups"], a["ratio"],
                                    a["counters"], a["ticket"], L.stream_ptr())

    cases = [(f"null {k}", lambda k=k: moments(**{k: None})) for k in ("p", "g", "m", "v", "segs", "groups", "counters", "partials", "ticket")]
    cases += [("ratio", lambda k=k: moments(**{k: None})) for k in ("ratio", "norm_w", "norm_u")]
    cases += [(f"null {k}", lambda k=k: apply(**{k: None})) for k in ("p", "m", "v", "segs", "groups", "ratio", "counters", "ticket")]
    cases += [("16-byte aligned", lambda k=k: moments(**{k: base[k] + 4})) for k in ("p", "g", "m", "v")]
    cases += [("16-byte aligned", lambda k=k: apply(**{k: base[k] + 4})) for k in ("p", "m", "v")]
    cases += [("partials must be 8-byte aligned", lambda: moments(partials=base["partials"] + 4)),
              ("ngroups", lambda: moments(ngroups=0)), ("ngroups", lambda: moments(groups=many, ngroups=L.ADAM_MAX_GROUPS + 1)),
              ("ngroups", lambda: apply(ngroups=0)), ("ngroups", lambda: apply(groups=many, ngroups=L.ADAM_MAX_GROUPS + 1)),
              ("nseg", lambda: moments(nseg=-1)), ("nseg", lambda: moments(nchunks=nseg - 1)), ("nseg", lambda: apply(nchunks=nseg - 1))]
    for what, fn in cases:
        rc = fn()
        err = L.lib.zsg_last_error().decode()
        assert rc == -1 and what in err, (what, rc, err)
    # nseg == 0 is not an error: nothing is launched, nothing written, no counter moves
    assert moments(nseg=0, nchunks=0) == 0 and apply(nseg=0, nchunks=0) == 0
    launched = _launches(L, lambda: [fn() for _, fn in cases] + [moments(nseg=0, nchunks=0), apply(nseg=0, nchunks=0)])
    assert launched == {}, launched
    assert all(torch.equal(a, b) for a, b in zip(keep, run.all_bits()))
    assert torch.equal(bits(part.view(torch.float32)), part0) and torch.equal(bits(st), st0)

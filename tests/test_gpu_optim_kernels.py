"""zsg_optim_step / zsg_optim_step_ema / zsg_optim_step_segments (csrc/optim.hip) at the C ABI: every rule (AdamW, Adam and AdamW with
amsgrad, SGD with momentum / Nesterov momentum / dampening, plain SGD) against torch.optim (foreach=False) on CPU copies, with the
tolerances of tests/test_gpu_adam_segments.py; the bit-identities the header promises (rule Adam = zsg_adam_step, AdamW at wd 0 = Adam, one
segment = the flat step, the riding average = step + zsg_ema_update, run to run); argument errors that launch and write nothing.  Flat
buffers sit between NaN guards with a payload, segments between NaN gaps: a write outside the range would change them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF          # a quiet NaN with a payload: any write of a computed value changes it
GUARD = 8                      # floats on either side of a flat buffer (keeps its 16-byte alignment)
ADAM, ADAMW, SGD, AMS = 0, 1, 2, 1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    assert (_lib.OPT_ADAM, _lib.OPT_ADAMW, _lib.OPT_SGD, _lib.OPT_AMSGRAD) == (ADAM, ADAMW, SGD, AMS)
    return _lib


def hp(lr=1e-2, b1=0.9, b2=0.99, eps=1e-8, wd=0.0, mom=0.0, damp=0.0, nest=False):
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, mom=mom, damp=damp, nest=nest)


# name -> (algo, flags, the hyperparameters of the flat tests, those of the three groups of the segmented test)
RULES = {
    "adamw": (ADAMW, 0, hp(wd=0.05), [hp(wd=0.01), hp(3e-3, 0.8, 0.999, 1e-6, 0.05), hp(5e-4, 0.95, 0.9, 1e-7)]),
    "adam_amsgrad": (ADAM, AMS, hp(wd=0.01), [hp(), hp(3e-3, 0.8, 0.999, 1e-6, 0.05), hp(5e-4, 0.95, 0.9, 1e-7)]),
    "adamw_amsgrad": (ADAMW, AMS, hp(wd=0.05), [hp(wd=0.01), hp(3e-3, 0.8, 0.999, 1e-6, 0.05), hp(5e-4, 0.95, 0.9, 1e-7)]),
    "sgd_momentum": (SGD, 0, hp(mom=0.9), [hp(mom=0.9), hp(3e-3, wd=0.05, mom=0.8), hp(5e-2, wd=1e-4)]),          # (a group without momentum)
    "sgd_nesterov": (SGD, 0, hp(wd=1e-4, mom=0.9, nest=True),
                     [hp(mom=0.9, nest=True), hp(3e-3, wd=0.05, mom=0.8, nest=True), hp(5e-2, wd=1e-4, mom=0.5, nest=True)]),
    "sgd_dampening": (SGD, 0, hp(mom=0.9, damp=0.1), [hp(mom=0.9, damp=0.1), hp(3e-3, wd=0.05, mom=0.8, damp=0.3), hp(5e-2, wd=1e-4, mom=0.7)]),
    "sgd_plain": (SGD, 0, hp(), [hp(), hp(3e-3, wd=0.05), hp(5e-2, wd=1e-4)]),
}
# the state buffers of a rule in the C ABI's order: (torch's state key, atol of the comparison) — rtol 1e-4 as test_gpu_adam_segments.py
ADAM_STATE = [("exp_avg", 1e-7), ("exp_avg_sq", 1e-9), ("max_exp_avg_sq", 1e-9)]


def state_of(algo, flags, hs):
    if algo == SGD:
        return [("momentum_buffer", 1e-7)] if any(h["mom"] != 0 for h in hs) else []
    return ADAM_STATE[:3 if flags & AMS else 2]


def group(L, h):
    return L.OptimGroup(h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["mom"], h["damp"], 1 if h["nest"] else 0)


def torch_group(algo, h):
    if algo == SGD:
        return dict(lr=h["lr"], momentum=h["mom"], dampening=h["damp"], weight_decay=h["wd"], nesterov=h["nest"])
    return dict(lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])


def torch_opt(algo, flags, groups):
    """groups: [(params, hyperparameters)]"""
    gs = [dict(params=ps, **torch_group(algo, h)) for ps, h in groups]
    if algo == SGD:
        return torch.optim.SGD(gs, lr=1e-3, foreach=False)
    return (torch.optim.AdamW if algo == ADAMW else torch.optim.Adam)(gs, amsgrad=bool(flags & AMS), foreach=False)


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


def ptr(t):
    return None if t is None else t.data_ptr()


class Flat:
    """p, three state buffers (used or not), the counter and an average, each between guards, from a seed"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.n, self.p0 = n, torch.randn(n, generator=g)
        self.wp, self.p = guarded(self.p0)
        self.ws, self.s = zip(*[guarded(torch.zeros(n)) for _ in range(3)])
        self.we, self.ema = guarded(torch.randn(n, generator=g))
        self.step2 = torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(self, L, algo, flags, h, gr, gs=1.0, ema_w=None, state=None):
        s = self.s if state is None else state
        head = (algo, flags, self.p.data_ptr(), gr.data_ptr(), ptr(s[0]), ptr(s[1]), ptr(s[2]), self.n, group(L, h), gs, self.step2.data_ptr())
        if ema_w is None:
            return L.lib.zsg_optim_step(*head, L.stream_ptr())
        return L.lib.zsg_optim_step_ema(*head, self.ema.data_ptr(), ema_w, L.stream_ptr())

    def all_bits(self):
        torch.cuda.synchronize()
        return [bits(t) for t in (self.wp, *self.ws, self.we)] + [self.step2.cpu()]


def grads(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for _ in range(steps)]


def run_flat(L, name, n, seed=7, steps=5, ema_ws=None, h=None):
    algo, flags, h0, _ = RULES[name]
    f = Flat(n, seed)
    for it, gr in enumerate(grads(n, steps, seed + 100)):
        L.check(f.call(L, algo, flags, h or h0, gr.cuda(), 0.5 if it == 2 else 1.0, None if ema_ws is None else ema_ws[it]), name)
    return f


SIZES = [1031, 3 * 16384 + 4099]          # 16-byte body + a 3-element tail in one block; 3 * ZSG_ADAM_CHUNK + 4099 (many blocks)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(RULES))
def test_flat_step_matches_torch(L, name, n):
    assert SIZES[1] == 3 * L.ADAM_CHUNK + 4099
    algo, flags, h, _ = RULES[name]
    f = run_flat(L, name, n)
    tp = torch.nn.Parameter(f.p0.clone())
    topt = torch_opt(algo, flags, [([tp], h)])
    for it, gr in enumerate(grads(n, 5, 107)):
        tp.grad = gr * (0.5 if it == 2 else 1.0)          # grad_scale = 0.5 on one step
        topt.step()
    torch.cuda.synchronize()
    assert f.step2.tolist() == [5, 0], "the counter reads 5 and the ticket 0"
    torch.testing.assert_close(f.p.cpu(), tp.detach(), rtol=1e-5, atol=1e-6)
    used = state_of(algo, flags, [h])
    for k, (key, atol) in enumerate(used):
        torch.testing.assert_close(f.s[k].cpu(), topt.state[tp][key], rtol=1e-4, atol=atol, msg=lambda m, key=key: f"{key}: {m}")
    for k in range(len(used), 3):
        assert not bool(f.s[k].any()), f"state buffer {k} is not this rule's and was written"
    assert all(guards_intact(w) for w in (f.wp, *f.ws)), "an element outside the buffer was written"
    # two runs from the same state: the same bits
    again = run_flat(L, name, n)
    assert all(torch.equal(a, b) for a, b in zip(f.all_bits(), again.all_bits()))


def seg_table(L, segs):
    """segs: [(off, len, group, counter)] -> (device table, nseg, nchunks)"""
    arr = (L.AdamSeg * len(segs))()
    chunk = 0
    for k, (off, n, gi, ci) in enumerate(segs):
        arr[k] = L.AdamSeg(off, n, gi, ci, chunk, 0)
        chunk += (n + L.ADAM_CHUNK - 1) // L.ADAM_CHUNK
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return tab, len(segs), chunk


@pytest.mark.parametrize("name", list(RULES))
def test_segments_match_torch_and_leave_gaps_alone(L, name):
    """the layout of test_gpu_adam_segments.py; the late segment is torch's parameter whose grad was None for two steps: its momentum
    buffer starts from its first gradient (dampening ignored), its vmax from 0, its bias correction from t = 1"""
    algo, flags, _, hps = RULES[name]
    g = torch.Generator().manual_seed(3)
    lens = [(7, 0), (4099, 1), (2 * L.ADAM_CHUNK + 5, 2), (1, 0), (33, 1), (520, 2)]
    late = 4                                    # this segment joins at step 2
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
        return torch.where(gap, nanv.expand(total), x).cuda()
    p = fresh(torch.randn(total, generator=g))
    st = [fresh(torch.zeros(total)) for _ in range(3)]
    gd = torch.full((total,), float("nan"), device="cuda")
    before = [t.view(torch.int32).clone() for t in (p, *st)]
    tps = [torch.nn.Parameter(p[o:o + n].detach().cpu().clone()) for (o, n, _, _) in segs]
    topt = torch_opt(algo, flags, [([tp for tp, s in zip(tps, segs) if s[2] == gi], h) for gi, h in enumerate(hps)])
    counters = torch.zeros(len(segs), dtype=torch.int32, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    gt = (L.OptimGroup * len(hps))(*[group(L, h) for h in hps])
    for it in range(5):
        on = [k for k in range(len(segs)) if k != late or it >= 2]
        tab, nseg, nch = seg_table(L, [segs[k] for k in on])
        for k, (o, n, _, _) in enumerate(segs):
            gr = torch.randn(n, generator=g)
            gd[o:o + n] = gr.cuda()
            tps[k].grad = gr.clone() if k in on else None          # torch's rule: no gradient, no step
        topt.step()
        L.check(L.lib.zsg_optim_step_segments(algo, flags, p.data_ptr(), gd.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                              tab.data_ptr(), nseg, nch, gt, len(hps), 1.0, counters.data_ptr(), ticket.data_ptr(),
                                              L.stream_ptr()), name)
    torch.cuda.synchronize()
    assert counters.tolist() == [5 if k != late else 3 for k in range(len(segs))] and int(ticket) == 0
    gapd = gap.cuda()
    for t, ref in zip((p, *st), before):
        assert torch.equal(t.view(torch.int32)[gapd], ref[gapd]), "an element outside the listed segments was written"
    used = state_of(algo, flags, hps)
    for k in range(len(used), 3):
        assert torch.equal(st[k].view(torch.int32), before[k + 1]), f"state buffer {k} is not this rule's and was written"
    for k, (o, n, gi, _) in enumerate(segs):
        torch.testing.assert_close(p[o:o + n].cpu(), tps[k].detach(), rtol=1e-5, atol=1e-6, msg=lambda m, k=k: f"segment {k}: {m}")
        tst = topt.state[tps[k]]
        for j, (key, atol) in enumerate(used):
            if tst.get(key) is None:          # a group without momentum: torch keeps no buffer, the kernel leaves its part alone
                assert algo == SGD and hps[gi]["mom"] == 0 and torch.equal(st[j].view(torch.int32)[o:o + n], before[j + 1][o:o + n])
                continue
            torch.testing.assert_close(st[j][o:o + n].cpu(), tst[key], rtol=1e-4, atol=atol, msg=lambda m, k=k, key=key: f"segment {k} {key}: {m}")
    if name == "sgd_momentum":
        assert any(topt.state[tp].get("momentum_buffer") is None for tp in tps), "the momentum-free group was meant to be covered"


@pytest.mark.parametrize("n", SIZES)
def test_rule_adam_gives_the_bits_of_zsg_adam_step(L, n):
    h = hp(2e-3, wd=1e-2)
    f = Flat(n, 5)
    pa = f.p0.cuda()
    ma, va = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step2 = torch.zeros(2, dtype=torch.int32, device="cuda")
    for it, gr in enumerate(grads(n, 4, 6)):
        gr = gr.cuda()
        L.check(L.lib.zsg_adam_step(pa.data_ptr(), gr.data_ptr(), ma.data_ptr(), va.data_ptr(), n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                                    0.5, step2.data_ptr(), L.stream_ptr()), "adam")
        L.check(f.call(L, ADAM, 0, h, gr, 0.5), "optim adam")
    torch.cuda.synchronize()
    assert step2.tolist() == f.step2.tolist() == [4, 0]
    for a, b in ((pa, f.p), (ma, f.s[0]), (va, f.s[1])):
        assert torch.equal(bits(a), bits(b))
    assert not bool(f.s[2].any())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("flags", [0, AMS])
def test_adamw_without_decay_gives_adams_bits(L, n, flags):
    h = hp(2e-3)
    fa, fw = Flat(n, 9), Flat(n, 9)
    for gr in grads(n, 4, 10):
        gr = gr.cuda()
        L.check(fa.call(L, ADAM, flags, h, gr), "adam")
        L.check(fw.call(L, ADAMW, flags, h, gr), "adamw")
    assert all(torch.equal(a, b) for a, b in zip(fa.all_bits(), fw.all_bits()))
    assert bool(fa.s[2].any()) == bool(flags)


@pytest.mark.parametrize("name", list(RULES))
def test_one_segment_one_group_is_the_flat_step_bit_for_bit(L, name):
    algo, flags, h, _ = RULES[name]
    n = SIZES[1]
    f, s = Flat(n, 5), Flat(n, 5)
    counters, ticket = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    tab, nseg, nch = seg_table(L, [(0, n, 0, 0)])
    gt = (L.OptimGroup * 1)(group(L, h))
    for gr in grads(n, 4, 6):
        gr = gr.cuda()
        L.check(f.call(L, algo, flags, h, gr, 0.5), name)
        L.check(L.lib.zsg_optim_step_segments(algo, flags, s.p.data_ptr(), gr.data_ptr(), s.s[0].data_ptr(), s.s[1].data_ptr(), s.s[2].data_ptr(),
                                              tab.data_ptr(), nseg, nch, gt, 1, 0.5, counters.data_ptr(), ticket.data_ptr(), L.stream_ptr()),
                name + " segments")
    torch.cuda.synchronize()
    assert f.step2.tolist() == [4, 0] and counters.tolist() == [4] and int(ticket) == 0
    assert all(torch.equal(a, b) for a, b in zip(f.all_bits()[:4], s.all_bits()[:4]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(RULES))
def test_riding_average_is_the_step_followed_by_ema_update(L, name, n):
    algo, flags, h, _ = RULES[name]
    ws = [1.0, 0.25, 0.25, 1.0]
    a, b = Flat(n, 11), Flat(n, 11)
    for w, gr in zip(ws, grads(n, 4, 12)):
        gr = gr.cuda()
        L.check(a.call(L, algo, flags, h, gr, ema_w=w), name + " ema")
        L.check(b.call(L, algo, flags, h, gr), name)
        L.check(L.lib.zsg_ema_update(b.ema.data_ptr(), b.p.data_ptr(), n, None, None, 0, w, L.stream_ptr()), "ema_update")
        if w == 1.0:
            torch.cuda.synchronize()
            assert torch.equal(bits(a.ema), bits(a.p)), "w = 1 stores p itself"
    assert all(torch.equal(x, y) for x, y in zip(a.all_bits(), b.all_bits()))
    assert guards_intact(a.we) and a.step2.tolist() == [4, 0]
    again = Flat(n, 11)
    for w, gr in zip(ws, grads(n, 4, 12)):
        L.check(again.call(L, algo, flags, h, gr.cuda(), ema_w=w), name + " ema")
    assert all(torch.equal(x, y) for x, y in zip(a.all_bits(), again.all_bits()))


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


def test_one_launch_per_flat_call_with_the_rules_bytes(L):
    n = 1031
    per = {"adamw": 28, "adam_amsgrad": 36, "adamw_amsgrad": 36, "sgd_momentum": 20, "sgd_nesterov": 20, "sgd_dampening": 20, "sgd_plain": 12}
    kind = {ADAM: "adam", ADAMW: "adamw", SGD: "sgd"}
    for name, (algo, flags, h, _) in RULES.items():
        f, gr = Flat(n, 1), grads(n, 1, 2)[0].cuda()
        for ema_w, suffix, extra in ((None, "", 0), (0.5, "_ema", 8)):
            got = _launches(L, lambda: [L.check(f.call(L, algo, flags, h, gr, ema_w=ema_w), name) for _ in range(3)])
            assert got == {f"optim_{kind[algo]}_step{suffix}": (3, 3.0 * n * (per[name] + extra))}, (name, got)


def test_plain_sgd_takes_null_state_and_argument_errors_write_nothing(L):
    n = 1031
    f, gr = Flat(n, 3), grads(n, 1, 4)[0].cuda()
    none = (None, None, None)
    assert f.call(L, SGD, 0, hp(wd=1e-4), gr, state=none) == 0
    assert f.call(L, SGD, 0, hp(wd=1e-4), gr, ema_w=0.5, state=none) == 0
    torch.cuda.synchronize()
    assert f.step2.tolist() == [2, 0] and not any(bool(s.any()) for s in f.s)
    keep = f.all_bits()
    tab, nseg, nch = seg_table(L, [(0, 16, 0, 0)])
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")

    def segments(algo, flags, hs, ngroups=None, s0=f.s[0]):
        gt = (L.OptimGroup * len(hs))(*[group(L, h) for h in hs])
        return L.lib.zsg_optim_step_segments(algo, flags, f.p.data_ptr(), gr.data_ptr(), ptr(s0), f.s[1].data_ptr(), f.s[2].data_ptr(),
                                             tab.data_ptr(), nseg, nch, gt, len(hs) if ngroups is None else ngroups, 1.0, cnt.data_ptr(),
                                             cnt[1:].data_ptr(), L.stream_ptr())
    odd = [f.s[0][1:], f.s[1], f.s[2]]          # (4 bytes off a 16-byte boundary)
    cases = [
        ("momentum buffer", lambda: f.call(L, SGD, 0, hp(mom=0.9), gr, state=none)),
        ("momentum buffer", lambda: segments(SGD, 0, [hp(), hp(mom=0.5)], s0=None)),
        ("null m", lambda: f.call(L, ADAMW, 0, hp(), gr, state=(None, f.s[1], None))),
        ("null m", lambda: f.call(L, ADAM, 0, hp(), gr, state=(f.s[0], None, None))),
        ("vmax", lambda: f.call(L, ADAM, AMS, hp(), gr, state=(f.s[0], f.s[1], None))),
        ("16-byte aligned", lambda: f.call(L, ADAMW, 0, hp(), gr, state=odd)),
        ("16-byte aligned", lambda: f.call(L, SGD, 0, hp(), gr[1:])),
        ("16-byte aligned", lambda: L.lib.zsg_optim_step_ema(SGD, 0, f.p.data_ptr(), gr.data_ptr(), None, None, None, n - 1, group(L, hp()), 1.0,
                                                             f.step2.data_ptr(), f.ema[1:].data_ptr(), 0.5, L.stream_ptr())),
        ("parameter groups", lambda: segments(ADAMW, 0, [hp()] * (L.ADAM_MAX_GROUPS + 1))),
        ("parameter groups", lambda: segments(SGD, 0, [hp()], ngroups=0)),
        ("ema_w", lambda: f.call(L, ADAMW, 0, hp(), gr, ema_w=1.5)),
        ("ema_w", lambda: f.call(L, SGD, 0, hp(), gr, ema_w=-0.1)),
        ("ema_w", lambda: f.call(L, SGD, 0, hp(), gr, ema_w=float("nan"))),
        ("nesterov", lambda: f.call(L, SGD, 0, hp(nest=True), gr)),
        ("nesterov", lambda: f.call(L, SGD, 0, hp(mom=0.9, damp=0.1, nest=True), gr)),
        ("nesterov", lambda: segments(SGD, 0, [hp(mom=0.9), hp(nest=True)])),
        ("unknown algorithm", lambda: f.call(L, 3, 0, hp(), gr)),
        ("unknown algorithm", lambda: segments(-1, 0, [hp()])),
        ("flags", lambda: f.call(L, ADAM, 2, hp(), gr)),
        ("amsgrad", lambda: f.call(L, SGD, AMS, hp(), gr)),
        ("step_count", lambda: L.lib.zsg_optim_step(SGD, 0, f.p.data_ptr(), gr.data_ptr(), None, None, None, n, group(L, hp()), 1.0, None,
                                                    L.stream_ptr())),
        ("null p or g", lambda: L.lib.zsg_optim_step(SGD, 0, f.p.data_ptr(), None, None, None, None, n, group(L, hp()), 1.0,
                                                     f.step2.data_ptr(), L.stream_ptr())),
        ("hyperparameters", lambda: L.lib.zsg_optim_step(SGD, 0, f.p.data_ptr(), gr.data_ptr(), None, None, None, n, None, 1.0,
                                                         f.step2.data_ptr(), L.stream_ptr())),
    ]
    for what, fn in cases:
        rc = fn()
        err = L.lib.zsg_last_error().decode()
        assert rc == -1 and what in err, (what, rc, err)
    launched = _launches(L, lambda: [fn() for _, fn in cases])
    assert launched == {}, launched
    assert all(torch.equal(a, b) for a, b in zip(keep, f.all_bits())) and cnt.tolist() == [0, 0]

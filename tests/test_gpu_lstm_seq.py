"""csrc/lstm_seq.hip through the C ABI: zsg_lstm_seq_fwd / zsg_lstm_seq_bwd (the query encoder's recurrence with a walk direction and
the state of every step as an output) and zsg_lang_pool_fwd / _bwd / _wgrad (mean and attention pooling of the padded output).

Method, helpers and rule are those of tests/test_gpu_lstm.py (make_inputs, length_patterns, valid_mask, the sentinel guards, the
NaN-filled gradient rows): the reference is a plain torch recurrence evaluated in float64 (seq_ref below: lstm_ref with a direction, the
padded output and its incoming gradient), the same code in float32 on the CPU is the yardstick, and each tensor must satisfy
    max|hip - fp64| <= 6 * max|cpu_fp32 - fp64| + floor,   floor = FLOOR[kind] * max|fp64|.
The kinds test_gpu_lstm.py already has (we, gates, cst, hprev, dgates) keep its FLOOR.  The new kinds get the largest CPU-fp32 error,
relative to the tensor's largest magnitude, over this file's parametrised cases (test_seq_forward_backward for hseq, test_pool for the
others); it is an error of the CPU reference, never of the kernels.

Largest relative error per kind over those cases, CPU fp32 / HIP, both against float64 (first run on an MI355X host):
  recurrence (test_seq_forward_backward)   we                 hseq               gates              cst                hprev              dgates
    H = 32                                 1.25e-7 / 1.84e-7  1.25e-7 / 1.84e-7  8.66e-8 / 1.52e-7  1.17e-7 / 1.33e-7  8.34e-8 / 9.71e-8  1.91e-7 / 2.09e-7
    H = 64                                 1.35e-7 / 1.49e-7  1.35e-7 / 2.20e-7  8.94e-8 / 1.90e-7  1.02e-7 / 1.80e-7  7.17e-8 / 9.95e-8  9.73e-8 / 2.09e-7
    H = 128                                1.19e-7 / 1.55e-7  1.45e-7 / 1.98e-7  1.40e-7 / 2.49e-7  1.23e-7 / 1.69e-7  7.14e-8 / 9.77e-8  1.90e-7 / 1.71e-7
    H = 256                                1.34e-7 / 2.50e-7  1.42e-7 / 2.50e-7  1.73e-7 / 4.23e-7  1.20e-7 / 2.44e-7  7.41e-8 / 1.41e-7  2.33e-7 / 3.73e-7
  pooling (test_pool)                      pooled             alpha              dhseq              ds                 dw
    D = 32                                 1.92e-7 / 2.58e-7  6.35e-8 / 1.01e-7  9.93e-8 / 1.56e-7  1.66e-7 / 1.16e-7  1.96e-7 / 1.47e-7
    D = 64                                 1.27e-7 / 1.31e-7  5.56e-8 / 9.24e-8  1.20e-7 / 9.13e-8  2.51e-7 / 1.67e-7  1.97e-7 / 2.32e-7
    D = 512                                2.58e-7 / 3.07e-7  1.65e-7 / 2.21e-7  1.78e-7 / 2.37e-7  3.84e-7 / 2.24e-7  3.41e-7 / 2.78e-7
The new floors are the largest CPU figure of their column, rounded up: hseq 1.5e-7, pooled 2.6e-7, alpha 1.7e-7, dhseq 1.8e-7, ds 3.9e-7,
dw 3.5e-7.  The HIP error never exceeded 0.31 of what the rule allows.  ds and dw of a one-token query are exactly 0 in float64 (alpha = 1): the
rule then allows nothing, and the kernels return exact zeros.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_lstm as TL  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_ops import Z, dev  # noqa: E402,F401

SENT = TL.SENT
FLOOR = dict(TL.FLOOR, hseq=1.5e-7, pooled=2.6e-7, alpha=1.7e-7, dhseq=1.8e-7, ds=3.9e-7, dw=3.5e-7)
MEAN, ATTN = 0, 1


def errors(what, kind, got, r64, r32, mask=None):
    """test_gpu_lstm.errors with this file's FLOOR: (hip error, cpu-fp32 error, allowed), printed before anything is asserted"""
    got = got.detach().cpu().double()
    if mask is not None:
        got, r64, r32 = got[mask], r64[mask], r32[mask]
    scale = float(r64.abs().max())
    e_hip, e_cpu = float((got - r64).abs().max()), float((r32.double() - r64).abs().max())
    tol = 6 * e_cpu + FLOOR[kind] * scale
    d = scale or 1.0          # (a tensor that is exactly 0 in float64 — ds and dw of a one-token query — must be exactly 0: tol = 0)
    print(f"ERR {what} {kind}: hip {e_hip:.3e} cpu_fp32 {e_cpu:.3e} scale {scale:.3e} hip_rel {e_hip / d:.3e} cpu_rel {e_cpu / d:.3e} tol {tol:.3e}")
    return e_hip, e_cpu, tol


def check_all(what, items):
    bad = []
    for kind, got, r64, r32, mask in items:
        e_hip, e_cpu, tol = errors(what, kind, got, r64, r32, mask)
        if not e_hip <= tol:          # (a NaN fails too)
            bad.append(f"{kind}: HIP err {e_hip:.3g} vs fp64 > 6 x CPU-fp32 err {e_cpu:.3g} + floor = {tol:.3g}")
    assert not bad, f"{what}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# the recurrence
# ------------------------------------------------------------------------------------------------------------------
def seq_ref(gin, w_hh, b_hh, h0, c0, rank, lens, reverse, dwe, dhseq):
    """test_gpu_lstm.lstm_ref with a walk direction: reverse consumes tokens len-1 .. 0; everything is stored at the TOKEN's position.
    hseq [B, T, H] is h of the step that consumed token t (0 at t >= len), we the state after the walk's last step (the starting state
    at len = 0); dgates = d(sum(we * dwe) + sum(hseq * dhseq)) / d gin.  dwe / dhseq may be None."""
    B, T, H4 = gin.shape
    H = H4 // 4
    gin.retain_grad()
    z = dict(dtype=gin.dtype)
    gates, cst, hprev = torch.zeros(B, T, H4, **z), torch.zeros(B, T, H, **z), torch.zeros(B, T, H, **z)
    we, rows = [], []
    for b in range(B):
        r = int(rank[b])
        n = max(0, min(int(lens[b]), T))
        h, c = h0[r:r + 1], c0[r:r + 1]
        out = [torch.zeros(1, H, **z)] * T
        for t in (range(n - 1, -1, -1) if reverse else range(n)):
            hprev[b, t] = h.detach()[0]
            pre = gin[b:b + 1, t] + h @ w_hh.t() + b_hh
            i, f, g, o = pre.chunk(4, dim=1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c = f * c + i * g
            h = o * torch.tanh(c)
            gates[b, t] = torch.cat([i, f, g, o], 1).detach()[0]
            cst[b, t] = c.detach()[0]
            out[t] = h
        we.append(h)
        rows.append(torch.cat(out, 0))
    we, hseq = torch.cat(we, 0), torch.stack(rows, 0)
    loss = (gin * 0).sum()
    if dwe is not None:
        loss = loss + (we * dwe).sum()
    if dhseq is not None:
        loss = loss + (hseq * dhseq).sum()
    loss.backward()
    return dict(we=we.detach(), hseq=hseq.detach(), gates=gates, cst=cst, hprev=hprev, dgates=gin.grad.detach())


def make_seq_inputs(H, B, T, seed, ld, off):
    """test_gpu_lstm.make_inputs plus the padded output's gradient: rows of ld, NaN outside [off, off + H)"""
    inp = TL.make_inputs(H, B, T, seed, ld, off)
    g = torch.Generator().manual_seed(seed + 7)
    dh = torch.full((B, T, ld), float("nan"), dtype=torch.float64)
    dh[:, :, off:off + H] = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    inp["dhseq"] = dh
    return inp


@functools.lru_cache(maxsize=None)
def seq_case(H, B, T, lens, reverse, off, use=("we", "hseq")):
    ld = 2 * H + 8
    inp = make_seq_inputs(H, B, T, 1000 * H + 10 * B + T + sum(lens) + reverse, ld, off)
    rank = O.sort_rank(torch.tensor(lens, dtype=torch.float32))
    out = {}
    for dt in (torch.float64, torch.float32):
        x = {k: v.float().to(dt) for k, v in inp.items()}
        out[dt] = seq_ref(x["gin"].requires_grad_(), x["w_hh"], x["b_hh"], x["h0"], x["c0"], rank, lens, reverse,
                          x["dwe"][:, off:off + H] if "we" in use else None, x["dhseq"][:, :, off:off + H] if "hseq" in use else None)
    return inp, out[torch.float64], out[torch.float32], rank, ld


class SeqRun:
    """One zsg_lstm_seq_fwd + zsg_lstm_seq_bwd pair.  Every output carries one more sample's worth of fill behind it."""

    def __init__(self, L, inp, qrank, lens, B, T, H, ld, off, reverse, use=("we", "hseq"), backward=True):
        f32 = {k: dev(v.float()) for k, v in inp.items()}
        self.gates = torch.full((B + 1, T, 4 * H), SENT, device="cuda")
        self.cst = torch.full((B + 1, T, H), SENT, device="cuda")
        self.hprev = torch.full((B + 1, T, H), SENT, device="cuda")
        self.we = torch.full((B + 1, ld), SENT, device="cuda")
        self.hseq = torch.full((B + 1, T, ld), SENT, device="cuda")
        self.dgates = torch.full((B + 1, T, 4 * H), float("nan"), device="cuda")
        self.qrank = dev(torch.tensor(qrank, dtype=torch.float32))
        self.lens = dev(torch.tensor(lens, dtype=torch.float32))
        st = L.stream_ptr()
        wp = self.we.data_ptr() if "we" in use else None
        hp = self.hseq.data_ptr() if "hseq" in use else None
        self.rc_fwd = L.lib.zsg_lstm_seq_fwd(f32["gin"].data_ptr(), f32["w_hh"].data_ptr(), f32["b_hh"].data_ptr(), f32["h0"].data_ptr(),
                                             f32["c0"].data_ptr(), self.qrank.data_ptr(), self.lens.data_ptr(), B, T, H, reverse,
                                             self.gates.data_ptr(), self.cst.data_ptr(), self.hprev.data_ptr(), hp, ld, off, wp, ld, off, st)
        self.rc_bwd = None
        if backward and self.rc_fwd == 0:
            self.rc_bwd = L.lib.zsg_lstm_seq_bwd(f32["dwe"].data_ptr() if "we" in use else None, ld, off,
                                                 f32["dhseq"].data_ptr() if "hseq" in use else None, ld, off, f32["w_hh"].data_ptr(),
                                                 self.gates.data_ptr(), self.cst.data_ptr(), f32["c0"].data_ptr(), self.qrank.data_ptr(),
                                                 self.lens.data_ptr(), B, T, H, reverse, self.dgates.data_ptr(), st)
        torch.cuda.synchronize()
        self.f32, self.B, self.T, self.H, self.off, self.use = f32, B, T, H, off, use

    def check_guards(self):
        B, H, o = self.B, self.H, self.off
        for name in ("gates", "cst", "hprev"):
            assert bool((getattr(self, name)[B] == SENT).all()), f"{name}: written behind the last sample"
        assert bool(torch.isnan(self.dgates[B]).all()), "dgates: written behind the last sample"
        we, hs = self.we.cpu(), self.hseq.cpu()
        if "we" in self.use:
            assert bool((we[B] == SENT).all()), "we: written behind the last sample"
            assert bool((we[:B, :o] == SENT).all()) and bool((we[:B, o + H:] == SENT).all()), "we: written outside its window"
            assert bool((we[:B, o:o + H] != SENT).all()), "we: part of its window not written"
        else:
            assert bool((we == SENT).all()), "we: written though NULL was passed"
        if "hseq" in self.use:
            assert bool((hs[B] == SENT).all()), "hseq: written behind the last sample"
            assert bool((hs[:B, :, :o] == SENT).all()) and bool((hs[:B, :, o + H:] == SENT).all()), "hseq: written outside its window"
            assert bool((hs[:B, :, o:o + H] != SENT).all()), "hseq: part of its window not written"
        else:
            assert bool((hs == SENT).all()), "hseq: written though NULL was passed"


def compare_seq(what, run, r64, r32, lens, T):
    m = TL.valid_mask([max(0, min(v, T)) for v in lens], T)
    B, H, o = run.B, run.H, run.off
    dg = run.dgates[:B].cpu()
    assert not bool(torch.isnan(dg).any()), f"{what}: dgates not written everywhere"
    assert bool((dg[~m] == 0.0).all()), f"{what}: dgates must be exactly 0 at t >= len"
    items = [(k, getattr(run, k)[:B], r64[k], r32[k], m) for k in ("gates", "cst", "hprev")] + [("dgates", dg, r64["dgates"], r32["dgates"], None)]
    if "we" in run.use:
        items.append(("we", run.we[:B, o:o + H], r64["we"], r32["we"], None))
    if "hseq" in run.use:
        hs = run.hseq[:B, :, o:o + H].cpu()
        assert bool((hs[~m] == 0.0).all()), f"{what}: hseq must be exactly 0 at t >= len"
        items.append(("hseq", hs, r64["hseq"], r32["hseq"], None))
    check_all(what, items)


def seq_cases():
    out = []
    for H in (32, 256):
        out.append((H, 1, 1, "full", (1,)))
        out += [(H, 5, 7, n, TL.length_patterns(5, 7)[n]) for n in ("full", "ones", "mixed")]
    out += [(H, 5, 7, "mixed", TL.length_patterns(5, 7)["mixed"]) for H in (64, 128)]
    return [c + (rev, off) for c in out for rev in (0, 1) for off in ("0", "H")]


SEQ_CASES = seq_cases()


@pytest.mark.parametrize("H,B,T,name,lens,reverse,off", SEQ_CASES, ids=[f"H{c[0]}-B{c[1]}-T{c[2]}-{c[3]}-rev{c[5]}-off{c[6]}" for c in SEQ_CASES])
def test_seq_forward_backward(Z, H, B, T, name, lens, reverse, off):
    """both outputs (the padded output and the end state) and both incoming gradients, in rows of 2H + 8 at window offset 0 or H"""
    L, ops = Z
    off = 0 if off == "0" else H
    inp, r64, r32, rank, ld = seq_case(H, B, T, lens, reverse, off)
    if name == "mixed":
        assert lens == (3, 7, 3, 7, 1) and rank.tolist() == [2, 0, 3, 1, 4]
    run = SeqRun(L, inp, lens, lens, B, T, H, ld, off, reverse)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards()
    compare_seq(f"H{H} B{B} T{T} {name} rev{reverse} off{off}", run, r64, r32, lens, T)
    if reverse and name == "mixed":          # the walks differ: token 0 of a 7-token query is the reverse walk's LAST step
        f64 = seq_case(H, B, T, lens, 0, off)[1]
        assert float((f64["hseq"] - r64["hseq"]).abs().max()) > 1e-2


@pytest.mark.parametrize("use", [("hseq",), ("we",)], ids=["seq_only", "end_only"])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("H", [32, 256])
def test_one_output_one_gradient(Z, H, reverse, use):
    """as the plans call it: mean / attn pass hseq and dhseq alone, final passes we and dwe alone; the other pointer is NULL"""
    L, ops = Z
    B, T, lens = 5, 7, (3, 7, 3, 7, 1)
    inp, r64, r32, rank, ld = seq_case(H, B, T, lens, reverse, H, use)
    run = SeqRun(L, inp, lens, lens, B, T, H, ld, H, reverse, use)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards()
    compare_seq(f"H{H} rev{reverse} {use[0]} only", run, r64, r32, lens, T)


@pytest.mark.parametrize("H", [32, 64, 128, 256])
def test_forward_walk_with_end_state_only_is_zsg_lstm(Z, H):
    """reverse = 0 with `we` alone: the bits of zsg_lstm_fwd / zsg_lstm_bwd on the same inputs"""
    L, ops = Z
    B, T, lens = 5, 7, (3, 7, 3, 7, 1)
    ld = 2 * H + 8
    inp = make_seq_inputs(H, B, T, 31 * H, ld, H)
    a = TL.Run(L, inp, lens, lens, B, T, H, ld, H)
    b = SeqRun(L, inp, lens, lens, B, T, H, ld, H, 0, ("we",))
    assert a.rc_fwd == a.rc_bwd == b.rc_fwd == b.rc_bwd == 0, L.lib.zsg_last_error().decode()
    b.check_guards()
    for k in ("we", "gates", "cst", "hprev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.dgates[:B], b.dgates[:B])


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("H", [32, 256])
def test_clamped_lengths_and_repeatability(Z, H, reverse):
    """lens = T + 3 runs T steps, bit-identical to lens = T; two runs of one call give the same bits"""
    L, ops = Z
    B, T = 5, 7
    lens = (T,) * B
    inp, r64, r32, rank, ld = seq_case(H, B, T, lens, reverse, 0)
    a = SeqRun(L, inp, lens, lens, B, T, H, ld, 0, reverse)
    b = SeqRun(L, inp, lens, (T + 3,) * B, B, T, H, ld, 0, reverse)
    c = SeqRun(L, inp, lens, lens, B, T, H, ld, 0, reverse)
    assert a.rc_fwd == a.rc_bwd == b.rc_fwd == b.rc_bwd == c.rc_fwd == c.rc_bwd == 0, L.lib.zsg_last_error().decode()
    b.check_guards()
    for k in ("we", "hseq", "gates", "cst", "hprev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert torch.equal(a.dgates[:B], b.dgates[:B]) and torch.equal(a.dgates[:B], c.dgates[:B])
    compare_seq(f"H{H} rev{reverse} lens T+3", b, r64, r32, lens, T)


@pytest.mark.parametrize("reverse", [0, 1])
def test_zero_length_row(Z, reverse):
    """len = 0 (never from the loader): the end state is the starting state, the padded output and dgates are 0 in that row"""
    L, ops = Z
    H, B, T, lens = 32, 3, 4, (2, 0, 4)
    inp, r64, r32, rank, ld = seq_case(H, B, T, lens, reverse, 0)
    run = SeqRun(L, inp, lens, lens, B, T, H, ld, 0, reverse)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards()
    assert torch.equal(run.we[1, :H], run.f32["h0"][int(rank[1])])
    assert not bool(run.hseq[1, :, :H].any()) and not bool(run.dgates[1].any())
    compare_seq(f"len0 rev{reverse}", run, r64, r32, lens, T)


def test_refused_calls(Z):
    L, ops = Z
    B, T, lens = 2, 3, (3, 2)
    H = 48
    inp = make_seq_inputs(H, B, T, 1, 2 * H + 8, 0)
    run = SeqRun(L, inp, lens, lens, B, T, H, 2 * H + 8, 0, 0, backward=False)
    assert run.rc_fwd == -1
    assert "32/64/128/256" in L.lib.zsg_last_error().decode() and "lstm_seq_fwd" in L.lib.zsg_last_error().decode()
    f, st = run.f32, L.stream_ptr()
    rc = L.lib.zsg_lstm_seq_bwd(f["dwe"].data_ptr(), 2 * H + 8, 0, f["dhseq"].data_ptr(), 2 * H + 8, 0, f["w_hh"].data_ptr(), run.gates.data_ptr(),
                                run.cst.data_ptr(), f["c0"].data_ptr(), run.qrank.data_ptr(), run.lens.data_ptr(), B, T, H, 0,
                                run.dgates.data_ptr(), st)
    assert rc == -1 and "lstm_seq_bwd" in L.lib.zsg_last_error().decode()
    H = 32
    inp = make_seq_inputs(H, B, T, 1, 2 * H + 8, 0)
    run = SeqRun(L, inp, lens, lens, B, T, H, 2 * H + 8, 0, 0, use=(), backward=False)
    assert run.rc_fwd == -1 and "hseq / we" in L.lib.zsg_last_error().decode()
    f = run.f32
    rc = L.lib.zsg_lstm_seq_bwd(None, 2 * H + 8, 0, None, 2 * H + 8, 0, f["w_hh"].data_ptr(), run.gates.data_ptr(), run.cst.data_ptr(),
                                f["c0"].data_ptr(), run.qrank.data_ptr(), run.lens.data_ptr(), B, T, H, 0, run.dgates.data_ptr(), st)
    assert rc == -1 and "dwe / dhseq" in L.lib.zsg_last_error().decode()
    torch.cuda.synchronize()
    for name in ("gates", "cst", "hprev", "we", "hseq"):
        assert bool((getattr(run, name) == SENT).all()), f"{name} touched by a refused call"
    assert bool(torch.isnan(run.dgates).all()), "dgates touched by a refused call"


# ------------------------------------------------------------------------------------------------------------------
# the pooling
# ------------------------------------------------------------------------------------------------------------------
def pool_ref(hseq, lens, w, mode, dwe):
    """we [B, D] from the padded output (autograd leaf) and, for attn, the scorer w (leaf); the saved weights alpha [B, T], the gradient
    ds of the scores (through a zero leaf added to them), dhseq and dw"""
    B, T, D = hseq.shape
    hseq.requires_grad_()
    if w is not None:
        w.requires_grad_()
    probe = torch.zeros(B, T, dtype=hseq.dtype, requires_grad=True)
    alpha = torch.zeros(B, T, dtype=hseq.dtype)
    rows = []
    for b in range(B):
        n = max(0, min(int(lens[b]), T))
        o = hseq[b, :n]
        if n == 0:
            rows.append(torch.zeros(D, dtype=hseq.dtype))
        elif mode == MEAN:
            rows.append(o.sum(0) / n)
        else:
            s = o @ w + probe[b, :n]
            a = torch.softmax(s - s.max().detach(), dim=0)
            alpha[b, :n] = a.detach()
            rows.append(a @ o)
    we = torch.stack(rows, 0)
    (we * dwe).sum().backward()
    out = dict(pooled=we.detach(), dhseq=hseq.grad.detach() if hseq.grad is not None else torch.zeros_like(hseq))
    if mode == ATTN:
        out.update(alpha=alpha, ds=probe.grad.detach(), dw=w.grad.detach())
    return out


@functools.lru_cache(maxsize=None)
def pool_case(D, B, T, lens, mode):
    g = torch.Generator().manual_seed(17 * D + B + T + sum(lens) + mode)
    m = TL.valid_mask([max(0, min(v, T)) for v in lens], T)
    hseq = (torch.rand(B, T, D, generator=g, dtype=torch.float64) * 2 - 1) * m.unsqueeze(2)          # |h| < 1, exactly 0 at t >= len
    # scores of order 1: an attention that is neither uniform nor one-hot
    w = torch.randn(D, generator=g, dtype=torch.float64) * 2.0 * D ** -0.5
    dwe = torch.randn(B, D, generator=g, dtype=torch.float64)
    inp = dict(hseq=hseq, w=w, dwe=dwe)
    out = {}
    for dt in (torch.float64, torch.float32):
        x = {k: v.float().to(dt) for k, v in inp.items()}
        out[dt] = pool_ref(x["hseq"], lens, x["w"] if mode == ATTN else None, mode, x["dwe"])
    return inp, out[torch.float64], out[torch.float32], m


POOL_LENS = {(1, 1): (1,), (5, 7): (3, 7, 3, 7, 1), (4, 20): (20, 0, 11, 25)}
POOL_CASES = [(D, B, T, mode) for D in (32, 64, 512) for (B, T) in POOL_LENS for mode in (MEAN, ATTN)]


@pytest.mark.parametrize("D,B,T,mode", POOL_CASES, ids=[f"D{c[0]}-B{c[1]}-T{c[2]}-{('mean', 'attn')[c[3]]}" for c in POOL_CASES])
def test_pool(Z, D, B, T, mode):
    L, ops = Z
    lens = POOL_LENS[(B, T)]
    inp, r64, r32, m = pool_case(D, B, T, lens, mode)
    what = f"D{D} B{B} T{T} {('mean', 'attn')[mode]}"
    f = {k: dev(v.float()) for k, v in inp.items()}
    ld = dev(torch.tensor(lens, dtype=torch.float32))
    we = torch.full((B + 1, D), SENT, device="cuda")
    alpha = torch.full((B + 1, T), SENT, device="cuda")
    dh = torch.full((B + 1, T, D), float("nan"), device="cuda")
    ds = torch.full((B + 1, T), float("nan"), device="cuda")
    st = L.stream_ptr()
    attn = mode == ATTN
    wp = f["w"].data_ptr() if attn else None

    def run(we, alpha, dh, ds):
        L.check(L.lib.zsg_lang_pool_fwd(f["hseq"].data_ptr(), ld.data_ptr(), wp, mode, B, T, D, we.data_ptr(), alpha.data_ptr() if attn else None, st), "pool_fwd")
        L.check(L.lib.zsg_lang_pool_bwd(f["dwe"].data_ptr(), f["hseq"].data_ptr(), ld.data_ptr(), wp, alpha.data_ptr() if attn else None, mode, B, T, D,
                                        dh.data_ptr(), ds.data_ptr() if attn else None, st), "pool_bwd")
        torch.cuda.synchronize()
    run(we, alpha, dh, ds)
    assert bool((we[B] == SENT).all()) and bool(torch.isnan(dh[B]).all()), "written behind the last sample"
    assert not bool(torch.isnan(dh[:B]).any()), "dhseq not written everywhere"
    assert bool((dh[:B].cpu()[~m] == 0.0).all()), "dhseq must be exactly 0 at t >= len"
    items = [("pooled", we[:B], r64["pooled"], r32["pooled"], None), ("dhseq", dh[:B], r64["dhseq"], r32["dhseq"], None)]
    for b, n in enumerate(lens):
        if n == 0:
            assert not bool(we[b].any()), "len = 0: we = 0"
    if attn:
        assert bool((alpha[B] == SENT).all()) and bool(torch.isnan(ds[B]).all()), "written behind the last sample"
        assert bool((alpha[:B].cpu()[~m] == 0.0).all()) and bool((ds[:B].cpu()[~m] == 0.0).all()), "alpha / ds must be exactly 0 at t >= len"
        dw = torch.full((D + 4,), SENT, device="cuda")
        L.check(L.lib.zsg_lang_pool_wgrad(ds.data_ptr(), f["hseq"].data_ptr(), B, T, D, dw.data_ptr(), 0, st), "pool_wgrad")
        pre = torch.randn(D, generator=torch.Generator().manual_seed(D)).cuda()
        acc = pre.clone()
        L.check(L.lib.zsg_lang_pool_wgrad(ds.data_ptr(), f["hseq"].data_ptr(), B, T, D, acc.data_ptr(), 1, st), "pool_wgrad")
        torch.cuda.synchronize()
        assert bool((dw[D:] == SENT).all()), "dw: written behind its D columns"
        assert torch.equal(acc, pre + dw[:D]), "accumulate = 1 adds the same sum to what is there"
        items += [("alpha", alpha[:B], r64["alpha"], r32["alpha"], None), ("ds", ds[:B], r64["ds"], r32["ds"], None),
                  ("dw", dw[:D], r64["dw"], r32["dw"], None)]
        if T > 1:
            # a kernel that ignores w computes the mean: the float64 attention output is far from it on the scale of what is allowed
            mean64 = pool_case(D, B, T, lens, MEAN)[1]["pooled"]
            e_cpu = float((r32["pooled"].double() - r64["pooled"]).abs().max())
            allowed = 6 * e_cpu + FLOOR["pooled"] * float(r64["pooled"].abs().max())
            gap = float((r64["pooled"] - mean64).abs().max())
            print(f"GAP {what}: attn - mean {gap:.3e}, allowed {allowed:.3e}")
            assert gap > 100 * allowed
    check_all(what, items)
    # the same bits on every run
    we2, alpha2, dh2, ds2 = torch.empty_like(we), torch.empty_like(alpha), torch.empty_like(dh), torch.empty_like(ds)
    run(we2, alpha2, dh2, ds2)
    assert torch.equal(we[:B], we2[:B]) and torch.equal(dh[:B], dh2[:B])
    if attn:
        assert torch.equal(alpha[:B], alpha2[:B]) and torch.equal(ds[:B], ds2[:B])


def test_pool_refused_calls(Z):
    L, ops = Z
    B, T, D = 2, 3, 32
    h, ln, o = torch.zeros(B, T, D, device="cuda"), dev(torch.tensor([3.0, 2.0])), torch.zeros(B, D, device="cuda")
    st = L.stream_ptr()
    assert L.lib.zsg_lang_pool_fwd(h.data_ptr(), ln.data_ptr(), None, ATTN, B, T, D, o.data_ptr(), None, st) == -1, "attn without w"
    assert L.lib.zsg_lang_pool_fwd(h.data_ptr(), ln.data_ptr(), None, 2, B, T, D, o.data_ptr(), None, st) == -1, "unknown mode"
    assert L.lib.zsg_lang_pool_fwd(None, ln.data_ptr(), None, MEAN, B, T, D, o.data_ptr(), None, st) == -1
    assert L.lib.zsg_lang_pool_bwd(o.data_ptr(), h.data_ptr(), ln.data_ptr(), None, None, ATTN, B, T, D, h.data_ptr(), None, st) == -1
    assert L.lib.zsg_lang_pool_bwd(o.data_ptr(), h.data_ptr(), ln.data_ptr(), None, None, MEAN, B, T, D, None, None, st) == -1
    assert L.lib.zsg_lang_pool_wgrad(None, h.data_ptr(), B, T, D, o.data_ptr(), 0, st) == -1
    torch.cuda.synchronize()

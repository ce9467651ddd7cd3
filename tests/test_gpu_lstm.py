"""csrc/lstm.hip through the C ABI at every compiled width (H = 32 / 64 / 128 with the recurrent weights in registers,
H = 256 reading them from memory in a 1024-thread block) and in both directions, against a plain torch recurrence.

Reference: lstm_ref() below, a loop of cell steps (gate order i, f, g, o as oracle.zsg_oracle.lstm_cell), evaluated in
float64 with the input projections `gin` as an autograd leaf: d(gate pre-activations) is gin.grad after we.backward(dwe),
the saved gates / cell states / previous hidden states are the loop's intermediates.  `gin` is generated directly, so only
the cases named *_through_gemm depend on zsg_conv_igemm / zsg_conv_wgrad / zsg_colsum.

Tolerance: the project's yardstick (tests/test_gpu_net.py).  The same recurrence runs in float32 on the CPU and each tensor
must satisfy   max|hip - fp64| <= 6 * max|cpu_fp32 - fp64| + floor,   floor = FLOOR[kind] * max|fp64|.
The floor covers the cases where the CPU happens to be exact (hprev of a one-step case is h0 itself: both errors are 0)
or nearly so, B = T = 1 above all.  Per kind of tensor it is the largest CPU-fp32 error, relative to the tensor's largest
magnitude, over the parametrised cases of test_forward_backward (wgrad: of test_forward_backward_through_gemm) as the
first run on an MI355X host printed them; it is never an error of the HIP kernels.

Observed on that run, largest relative error per width, CPU fp32 / HIP, both against float64:
  recurrence alone   we                gates             cst               hprev             dgates
    H = 32           1.65e-7 / 1.84e-7  2.05e-7 / 2.09e-7  1.70e-7 / 1.50e-7  1.40e-7 / 1.57e-7  2.59e-7 / 2.59e-7
    H = 64           1.54e-7 / 2.21e-7  2.89e-7 / 2.62e-7  1.23e-7 / 1.58e-7  1.57e-7 / 1.66e-7  1.77e-7 / 2.97e-7
    H = 128          1.82e-7 / 2.50e-7  3.57e-7 / 3.59e-7  1.39e-7 / 1.96e-7  1.79e-7 / 2.02e-7  1.74e-7 / 2.83e-7
    H = 256          2.96e-7 / 3.01e-7  6.25e-7 / 5.71e-7  1.47e-7 / 2.29e-7  1.56e-7 / 2.45e-7  2.50e-7 / 2.97e-7
  through the GEMMs  we                gates             dgates            weight / bias gradients
    H = 32           3.51e-7 / 6.96e-7  4.40e-7 / 5.56e-7  2.39e-7 / 2.70e-7  3.93e-7 / 2.95e-7
    H = 64           2.96e-7 / 3.53e-7  6.17e-7 / 5.52e-7  2.67e-7 / 3.25e-7
    H = 128          1.97e-7 / 2.75e-7  4.14e-7 / 4.94e-7  1.51e-7 / 2.02e-7
    H = 256          1.48e-7 / 2.36e-7  3.24e-7 / 5.36e-7  1.64e-7 / 1.76e-7  2.65e-7 / 2.48e-7
The HIP error never exceeded 0.39 of what the rule allows.  (The CPU figures depend on the host's BLAS and thread count:
another machine gave 3.5e-7 instead of 6.25e-7 for the gates at H = 256, which is why the floor is a recorded constant.)
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_ops import WS, Z, dev  # noqa: E402,F401

WIDTHS = (32, 64, 128, 256)
SENT = -777.0          # no LSTM output reaches it (|gates|, |h| <= 1; |c| <= |c0| + T)
FLOOR = {"we": 3.0e-7, "gates": 6.3e-7, "cst": 1.7e-7, "hprev": 1.8e-7, "dgates": 2.6e-7, "wgrad": 4.0e-7}


# ------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------
def lstm_ref(gin, w_hh, b_hh, h0, c0, rank, lens, dwe):
    """One direction of the query encoder as a loop of cell steps.  gin [B, T, 4H] = x_t W_ih^T + b_ih; sample b starts
    from row rank[b] of h0 / c0 [B, H] and runs lens[b] steps; we [B, H] is its last hidden state.  Returns we, the
    activated gates [B, T, 4H], the cell states and the hidden states each step started from [B, T, H] (zero at
    t >= lens[b]) and dgates = d(sum(we * dwe)) / d(gin + h W_hh^T + b_hh), which is d / d gin."""
    B, T, H4 = gin.shape
    H = H4 // 4
    gin.retain_grad()
    gates, cst, hprev = torch.zeros(B, T, H4, dtype=gin.dtype), torch.zeros(B, T, H, dtype=gin.dtype), torch.zeros(B, T, H, dtype=gin.dtype)
    we = []
    for b in range(B):
        r = int(rank[b])
        h, c = h0[r:r + 1], c0[r:r + 1]
        for t in range(int(lens[b])):
            hprev[b, t] = h.detach()[0]
            pre = gin[b:b + 1, t] + h @ w_hh.t() + b_hh
            i, f, g, o = pre.chunk(4, dim=1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c = f * c + i * g
            h = o * torch.tanh(c)
            gates[b, t] = torch.cat([i, f, g, o], 1).detach()[0]
            cst[b, t] = c.detach()[0]
        we.append(h)
    we = torch.cat(we, 0)
    we.backward(dwe)
    return dict(we=we.detach(), gates=gates, cst=cst, hprev=hprev, dgates=gin.grad.detach())


def make_inputs(H, B, T, seed, we_ld, we_off):
    """float64 inputs of one direction; rows of h0 / c0 grow with their index, so a wrong rank is a large error"""
    g = torch.Generator().manual_seed(seed)
    k = H ** -0.5
    rows = torch.arange(1, B + 1, dtype=torch.float64).view(B, 1)
    dwe = torch.full((B, we_ld), float("nan"), dtype=torch.float64)          # the backward may read its window only
    dwe[:, we_off:we_off + H] = torch.randn(B, H, generator=g, dtype=torch.float64)
    return dict(gin=torch.randn(B, T, 4 * H, generator=g, dtype=torch.float64),
                w_hh=(torch.rand(4 * H, H, generator=g, dtype=torch.float64) * 2 - 1) * k,
                b_hh=(torch.rand(4 * H, generator=g, dtype=torch.float64) * 2 - 1) * k,
                h0=0.1 * rows * torch.randn(B, H, generator=g, dtype=torch.float64),
                c0=0.1 * rows * torch.randn(B, H, generator=g, dtype=torch.float64), dwe=dwe)


def both_refs(inp, lens, we_off, H):
    """the recurrence in float64 (the truth) and in float32 on the CPU (the yardstick), from the float32-rounded inputs"""
    rank = O.sort_rank(torch.tensor(lens, dtype=torch.float32))
    out = {}
    for dt in (torch.float64, torch.float32):
        x = {k: v.float().to(dt) for k, v in inp.items()}
        out[dt] = lstm_ref(x["gin"].requires_grad_(), x["w_hh"], x["b_hh"], x["h0"], x["c0"], rank, lens, x["dwe"][:, we_off:we_off + H])
    return out[torch.float64], out[torch.float32], rank


@functools.lru_cache(maxsize=None)
def case_data(H, B, T, lens, we_off=0):
    we_ld = 2 * H + 8
    inp = make_inputs(H, B, T, 1000 * H + 10 * B + T + sum(lens), we_ld, we_off)
    r64, r32, rank = both_refs(inp, lens, we_off, H)
    return inp, r64, r32, rank, we_ld


def errors(what, kind, got, r64, r32, mask=None):
    """(hip error, cpu-fp32 error, allowed) of one tensor, printed before anything is asserted"""
    got = got.detach().cpu().double()
    if mask is not None:
        got, r64, r32 = got[mask], r64[mask], r32[mask]
    scale = float(r64.abs().max())
    e_hip, e_cpu = float((got - r64).abs().max()), float((r32.double() - r64).abs().max())
    tol = 6 * e_cpu + FLOOR[kind] * scale
    print(f"ERR {what} {kind}: hip {e_hip:.3e} cpu_fp32 {e_cpu:.3e} scale {scale:.3e} hip_rel {e_hip / scale:.3e} cpu_rel {e_cpu / scale:.3e} tol {tol:.3e}")
    return e_hip, e_cpu, tol


def check_all(what, items):
    bad = []
    for kind, got, r64, r32, mask in items:
        e_hip, e_cpu, tol = errors(what, kind, got, r64, r32, mask)
        if not e_hip <= tol:          # (a NaN fails too)
            bad.append(f"{kind}: HIP err {e_hip:.3g} vs fp64 > 6 x CPU-fp32 err {e_cpu:.3g} + floor = {tol:.3g}")
    assert not bad, f"{what}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------------------------
class Run:
    """One zsg_lstm_fwd + zsg_lstm_bwd call pair.  Every output carries one more sample's worth of fill behind it."""

    def __init__(self, L, inp, qrank, lens, B, T, H, we_ld, we_off, fill=SENT, backward=True):
        f32 = {k: dev(v.float()) for k, v in inp.items()}
        self.gates = torch.full((B + 1, T, 4 * H), fill, device="cuda")
        self.cst = torch.full((B + 1, T, H), fill, device="cuda")
        self.hprev = torch.full((B + 1, T, H), fill, device="cuda")
        self.we = torch.full((B + 1, we_ld), SENT, device="cuda")
        self.dgates = torch.full((B + 1, T, 4 * H), float("nan"), device="cuda")
        self.qrank = dev(torch.tensor(qrank, dtype=torch.float32))
        self.lens = None if lens is None else dev(torch.tensor(lens, dtype=torch.float32))
        lp = None if lens is None else self.lens.data_ptr()
        st = L.stream_ptr()
        self.rc_fwd = L.lib.zsg_lstm_fwd(f32["gin"].data_ptr(), f32["w_hh"].data_ptr(), f32["b_hh"].data_ptr(), f32["h0"].data_ptr(),
                                         f32["c0"].data_ptr(), self.qrank.data_ptr(), lp, B, T, H, self.gates.data_ptr(), self.cst.data_ptr(),
                                         self.hprev.data_ptr(), self.we.data_ptr(), we_ld, we_off, st)
        self.rc_bwd = None
        if backward and self.rc_fwd == 0:
            self.rc_bwd = L.lib.zsg_lstm_bwd(f32["dwe"].data_ptr(), we_ld, we_off, f32["w_hh"].data_ptr(), self.gates.data_ptr(),
                                             self.cst.data_ptr(), f32["c0"].data_ptr(), self.qrank.data_ptr(), lp, B, T, H,
                                             self.dgates.data_ptr(), st)
        torch.cuda.synchronize()
        self.f32, self.B, self.H, self.we_off = f32, B, H, we_off

    def check_guards(self, fill=SENT):
        B, H, o = self.B, self.H, self.we_off
        for name in ("gates", "cst", "hprev"):
            assert bool((getattr(self, name)[B] == fill).all()), f"{name}: written behind the last sample"
        assert bool(torch.isnan(self.dgates[B]).all()), "dgates: written behind the last sample"
        we = self.we.cpu()
        assert bool((we[B] == SENT).all()), "we: written behind the last sample"
        assert bool((we[:B, :o] == SENT).all()) and bool((we[:B, o + H:] == SENT).all()), "we: written outside [we_off, we_off + H)"
        assert bool((we[:B, o:o + H] != SENT).all()), "we: part of [we_off, we_off + H) not written"

    def window(self):
        return self.we[:self.B, self.we_off:self.we_off + self.H]


def valid_mask(lens, T):
    return torch.arange(T).view(1, T) < torch.tensor(lens).view(-1, 1)


def compare(what, run, r64, r32, lens, T):
    m = valid_mask(lens, T)
    B = run.B
    dg = run.dgates[:B].cpu()
    assert not bool(torch.isnan(dg).any()), f"{what}: dgates not written everywhere"
    assert bool((dg[~m] == 0.0).all()), f"{what}: dgates must be exactly 0 at t >= len"
    check_all(what, [("we", run.window(), r64["we"], r32["we"], None)] +
              [(k, getattr(run, k)[:B], r64[k], r32[k], m) for k in ("gates", "cst", "hprev")] +
              [("dgates", dg, r64["dgates"], r32["dgates"], None)])


def length_patterns(B, T):
    """all equal (every pair ties: identity rank), all 1, strictly ascending (the rank is a full reversal), strictly descending,
    and ties placed so that the stable order matters"""
    if B == 1:
        return {"full": (T,)} if T == 1 else {"full": (T,), "ones": (1,), "mid": (T // 2 + 1,)}
    asc = tuple(T - B + 1 + b for b in range(B))
    mixed = tuple(min(v, T) for v in (3, 7, 3, 7, 1, T, 2, T, 5, 5, 1, 7, 3, 2, T, 6)[:B])
    return {"full": (T,) * B, "ones": (1,) * B, "asc": asc, "desc": asc[::-1], "mixed": mixed}


CASES = [(H, B, T, name, lens) for H in WIDTHS for B, T in ((1, 1), (1, 20), (5, 7), (16, 20)) for name, lens in length_patterns(B, T).items()]


@pytest.mark.parametrize("H,B,T,name,lens", CASES, ids=[f"H{c[0]}-B{c[1]}-T{c[2]}-{c[3]}" for c in CASES])
def test_forward_backward(Z, H, B, T, name, lens):
    L, ops = Z
    inp, r64, r32, rank, we_ld = case_data(H, B, T, lens)
    if name == "mixed" and B == 5:
        assert lens == (3, 7, 3, 7, 1) and rank.tolist() == [2, 0, 3, 1, 4]          # equal lengths keep their batch order
    if name == "asc":
        assert rank.tolist() == list(range(B - 1, -1, -1))
    if name in ("full", "ones", "desc"):
        assert rank.tolist() == list(range(B))
    run = Run(L, inp, lens, lens, B, T, H, we_ld, 0)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards()
    compare(f"H{H} B{B} T{T} {name}", run, r64, r32, lens, T)


@pytest.mark.parametrize("we_off", ["0", "H", "4"])
@pytest.mark.parametrize("H", WIDTHS)
def test_output_window(Z, H, we_off):
    """we / dwe rows are we_ld = 2H + 8 apart and only [we_off, we_off + H) of each belongs to this direction"""
    L, ops = Z
    B, T, lens = 5, 7, (3, 7, 3, 7, 1)
    off = {"0": 0, "H": H, "4": 4}[we_off]
    inp, r64, r32, rank, we_ld = case_data(H, B, T, lens, off)
    run = Run(L, inp, lens, lens, B, T, H, we_ld, off)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards()
    compare(f"H{H} we_off {off}", run, r64, r32, lens, T)


@pytest.mark.parametrize("H", WIDTHS)
def test_lengths_beyond_T_are_clamped(Z, H):
    """lens[b] = T + 3 runs T steps (the kernels clamp len to [0, T]): bit-identical to lens[b] = T"""
    L, ops = Z
    B, T = 5, 7
    lens = (T,) * B
    inp, r64, r32, rank, we_ld = case_data(H, B, T, lens)
    a = Run(L, inp, lens, lens, B, T, H, we_ld, 0)
    b = Run(L, inp, lens, (T + 3,) * B, B, T, H, we_ld, 0)
    assert a.rc_fwd == a.rc_bwd == b.rc_fwd == b.rc_bwd == 0, L.lib.zsg_last_error().decode()
    b.check_guards()
    for k in ("we", "gates", "cst", "hprev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.dgates[:B], b.dgates[:B])
    compare(f"H{H} lens T+3", b, r64, r32, lens, T)


@pytest.mark.parametrize("B,T", [(5, 7), (16, 20)])
@pytest.mark.parametrize("H", WIDTHS)
def test_reverse_direction(Z, H, B, T):
    """The reverse direction as _lower_lstm issues it: zsg_lstm_gather_last picks x[len - 1], then ONE cell step (T = 1,
    lens = NULL) from row rank[b] of the second half of h0 / c0 into [H, 2H) of we; the rank still comes from the lengths."""
    L, ops = Z
    E = 300
    lens = length_patterns(B, T)["mixed"]
    g = torch.Generator().manual_seed(H + B)
    qvec = dev(torch.randn(B, T, E, generator=g))
    st = L.stream_ptr()
    for ql in (lens, tuple(v + (T if i % 2 else 0) for i, v in enumerate(lens))):          # lengths beyond T read step T - 1
        xlast = torch.full((B + 1, E), SENT, device="cuda")
        qd = dev(torch.tensor(ql, dtype=torch.float32))
        assert L.lib.zsg_lstm_gather_last(qvec.data_ptr(), qd.data_ptr(), B, T, E, xlast.data_ptr(), st) == 0
        want = qvec[torch.arange(B), torch.tensor([min(v, T) - 1 for v in ql])]
        assert torch.equal(xlast[:B], want) and bool((xlast[B] == SENT).all()), "gather_last must copy qvec[b, len - 1] bit for bit"
    we_ld, we_off = 2 * H + 8, H
    inp = make_inputs(H, B, 1, 77 * H + B, we_ld, we_off)
    rank = O.sort_rank(torch.tensor(lens, dtype=torch.float32))
    assert rank.tolist() != list(range(B))
    r64, r32 = [lstm_ref(x["gin"].requires_grad_(), x["w_hh"], x["b_hh"], x["h0"], x["c0"], rank, (1,) * B, x["dwe"][:, we_off:we_off + H])
                for x in ({k: v.float().to(dt) for k, v in inp.items()} for dt in (torch.float64, torch.float32))]
    run = Run(L, inp, lens, None, B, 1, H, we_ld, we_off)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards()
    compare(f"H{H} B{B} reverse", run, r64, r32, (1,) * B, 1)


@pytest.mark.parametrize("H", [48, 100, 512])
def test_unsupported_width_is_refused(Z, H):
    L, ops = Z
    B, T = 2, 3
    inp = make_inputs(H, B, T, 1, 2 * H + 8, 0)
    run = Run(L, inp, (3, 2), (3, 2), B, T, H, 2 * H + 8, 0, backward=False)
    assert run.rc_fwd == -1
    assert "32/64/128/256" in L.lib.zsg_last_error().decode() and "lstm_fwd" in L.lib.zsg_last_error().decode()
    f = run.f32
    rc = L.lib.zsg_lstm_bwd(f["dwe"].data_ptr(), 2 * H + 8, 0, f["w_hh"].data_ptr(), run.gates.data_ptr(), run.cst.data_ptr(), f["c0"].data_ptr(),
                            run.qrank.data_ptr(), run.lens.data_ptr(), B, T, H, run.dgates.data_ptr(), L.stream_ptr())
    assert rc == -1
    assert "32/64/128/256" in L.lib.zsg_last_error().decode() and "lstm_bwd" in L.lib.zsg_last_error().decode()
    torch.cuda.synchronize()
    for name in ("gates", "cst", "hprev", "we"):
        assert bool((getattr(run, name) == SENT).all()), f"{name} touched by a refused call"
    assert bool(torch.isnan(run.dgates).all()), "dgates touched by a refused call"


def test_null_pointer_is_refused(Z):
    L, ops = Z
    H, B, T = 32, 2, 3
    run = Run(L, make_inputs(H, B, T, 1, 2 * H + 8, 0), (3, 2), (3, 2), B, T, H, 2 * H + 8, 0)
    assert run.rc_fwd == 0 and run.rc_bwd == 0
    f, st = run.f32, L.stream_ptr()
    fwd = [f["gin"], f["w_hh"], f["b_hh"], f["h0"], f["c0"], run.qrank, run.lens, B, T, H, run.gates, run.cst, run.hprev, run.we, 2 * H + 8, 0]
    bwd = [f["dwe"], 2 * H + 8, 0, f["w_hh"], run.gates, run.cst, f["c0"], run.qrank, run.lens, B, T, H, run.dgates]
    for fn, args, optional in ((L.lib.zsg_lstm_fwd, fwd, 6), (L.lib.zsg_lstm_bwd, bwd, 8)):
        for i, a in enumerate(args):
            if isinstance(a, torch.Tensor) and i != optional:          # (lens is the one optional pointer)
                call = [None if j == i else (x.data_ptr() if isinstance(x, torch.Tensor) else x) for j, x in enumerate(args)]
                assert fn(*call, st) == -1, f"{fn.__name__}: NULL argument {i} accepted"
                assert "null argument" in L.lib.zsg_last_error().decode()
    q = dev(torch.zeros(B, T, 8))
    o = torch.zeros(B, 8, device="cuda")
    for call in ((None, run.lens.data_ptr(), B, T, 8, o.data_ptr()), (q.data_ptr(), None, B, T, 8, o.data_ptr()), (q.data_ptr(), run.lens.data_ptr(), B, T, 8, None)):
        assert L.lib.zsg_lstm_gather_last(*call, st) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# with the MFMA GEMMs around the recurrence, as the plan runs them
# ------------------------------------------------------------------------------------------------------------------
def encoder_ref(p, qvec, h0, c0, rank, lens, dwe, dt):
    """fp64 / fp32 reference of one direction from the word vectors on: parameters are leaves, their .grad the result"""
    p = {k: v.float().to(dt).requires_grad_() for k, v in p.items()}
    gin = qvec.float().to(dt) @ p["w_ih"].t() + p["b_ih"]
    r = lstm_ref(gin, p["w_hh"], p["b_hh"], h0.float().to(dt), c0.float().to(dt), rank, lens, dwe.float().to(dt))
    r.update({"d" + k: v.grad for k, v in p.items()})
    return r


GEMM_LENS = (3, 7, 3, 7, 1)


@functools.lru_cache(maxsize=None)
def gemm_case(H):
    B, T, E, lens, H4 = 5, 7, 300, GEMM_LENS, 4 * H
    g = torch.Generator().manual_seed(5 * H)
    k = H ** -0.5
    p = {n: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k for n, s in (("w_ih", (H4, E)), ("b_ih", (H4,)), ("w_hh", (H4, H)), ("b_hh", (H4,)))}
    qvec = torch.randn(B, T, E, generator=g, dtype=torch.float64) * 0.35
    rows = torch.arange(1, B + 1, dtype=torch.float64).view(B, 1)
    h0, c0 = 0.1 * rows * torch.randn(B, H, generator=g, dtype=torch.float64), 0.1 * rows * torch.randn(B, H, generator=g, dtype=torch.float64)
    dwe = torch.randn(B, H, generator=g, dtype=torch.float64)
    rank = O.sort_rank(torch.tensor(lens, dtype=torch.float32))
    r64, r32 = (encoder_ref(p, qvec, h0, c0, rank, lens, dwe, dt) for dt in (torch.float64, torch.float32))
    return p, qvec, h0, c0, dwe, r64, r32


@pytest.mark.parametrize("H", WIDTHS)
def test_forward_backward_through_gemm(Z, H):
    """E = 300 word vectors -> zsg_conv_igemm (input projection) -> zsg_lstm_fwd -> zsg_lstm_bwd; at H = 32 and 256 also the
    weight / bias gradients through zsg_conv_wgrad / zsg_colsum, against float64 autograd."""
    L, ops = Z
    B, T, E, lens, H4 = 5, 7, 300, GEMM_LENS, 4 * H
    p, qvec, h0, c0, dwe, r64, r32 = gemm_case(H)
    st = L.stream_ptr()
    xin = dev(qvec.float())
    gin = torch.empty(B, T, H4, device="cuda")
    src = ops.TView(xin.view(-1), B, E, E, [ops.Level(0, 1, T, T * E)])
    gv = ops.TView(gin.view(-1), B, H4, H4, [ops.Level(0, 1, T, T * H4)])
    w = {n: dev(v.float()) for n, v in p.items()}
    L.check(L.lib.zsg_conv_igemm(C.byref(ops.fwd_desc(src, gv, E, H4, 1, 1, 0, 1, wC=E)), xin.data_ptr(), w["w_ih"].data_ptr(), gin.data_ptr(),
                                 w["b_ih"].data_ptr(), None, None, None, st), "lstm_in")
    inp = dict(gin=gin.cpu(), w_hh=p["w_hh"], b_hh=p["b_hh"], h0=h0, c0=c0, dwe=dwe)
    run = Run(L, inp, lens, lens, B, T, H, H, 0, fill=0.0)          # (rows at t >= len stay 0, as in the plan's zero-filled buffers)
    assert run.rc_fwd == 0 and run.rc_bwd == 0, L.lib.zsg_last_error().decode()
    run.check_guards(fill=0.0)
    compare(f"H{H} gemm", run, r64, r32, lens, T)
    if H not in (32, 256):
        return
    dg, hprev = run.dgates[:B].contiguous(), run.hprev[:B].contiguous()
    dgv = ops.TView(dg.view(-1), B, H4, H4, [ops.Level(0, 1, T, T * H4)])
    dwih, dwhh, db = torch.zeros(H4, E, device="cuda"), torch.zeros(H4, H, device="cuda"), torch.zeros(H4, device="cuda")
    L.check(L.lib.zsg_conv_wgrad(C.byref(ops.fwd_desc(src, dgv, E, H4, 1, 1, 0, 1, wC=E)), xin.data_ptr(), dg.data_ptr(), dwih.data_ptr(), 0,
                                 WS.data_ptr(), WS.numel() * 4, st), "w_ih")
    hp = ops.TView(hprev.view(-1), B, H, H, [ops.Level(0, 1, T, T * H)])
    L.check(L.lib.zsg_conv_wgrad(C.byref(ops.fwd_desc(hp, dgv, H, H4, 1, 1, 0, 1, wC=H)), hprev.data_ptr(), dg.data_ptr(), dwhh.data_ptr(), 0,
                                 WS.data_ptr(), WS.numel() * 4, st), "w_hh")
    L.check(L.lib.zsg_colsum(dg.data_ptr(), 1, 0, B * T, H4, 0, H4, db.data_ptr(), 0, st), "bias")
    torch.cuda.synchronize()
    check_all(f"H{H} gemm", [("wgrad", dwih, r64["dw_ih"], r32["dw_ih"], None), ("wgrad", dwhh, r64["dw_hh"], r32["dw_hh"], None),
                             ("wgrad", db, r64["db_ih"], r32["db_ih"], None), ("wgrad", db, r64["db_hh"], r32["db_hh"], None)])

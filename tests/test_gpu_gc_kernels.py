"""csrc/gcblock.hip through the C ABI: zsg_head_gc_fwd and zsg_head_gc_bwd (include/zsg.h), every output between canaries.

IDENTITIES that need no tolerance: fc2 = 0 gives y = x and dx = g (torch.equal; dW2 / db2 are still checked against the reference);
two runs give the same bits; bad arguments are refused by name with nothing written.  key = 0 makes c the row mean (bound: an fp32 sum
of P terms and one division, (P + 1) * 2^-24 * max |x|); logits of magnitude 80 leave every output finite.
RANDOM inputs are compared with tests/gc_ref.py on the same fp32 operands: the truth is its float64 evaluation (backward by autograd),
the yardstick its float32 CPU evaluation, and each tensor of the GPU (y, dx, the seven gradients) may be 4 x as far from the truth as
the yardstick is (max-abs): the kernels may reorder sums but not lose precision.  The measured figures: profiles/head_ctx_parity_measured.txt.
Geometries: a single 1 x 1 level (a softmax over one row), 3 x 3, 5 x 7 (fills no wave's share and no chunk), one level of 63 / 64 / 65
rows (the kernels' chunk is 64 rows), a mixed pyramid ending in 2 x 2 and 1 x 1, each at Q = 1 and 3, and the 300-pixel pyramid once."""
import functools

import pytest
import torch

import gc_ref as GR

pytestmark = pytest.mark.gpu

N, M = 256, 64
CHUNK = 64                      # GC_CH of csrc/gcblock.hip
ST_MAX, ST_DEN, ST_VAR, ST_RSTD, ST_C, ST_UHAT, ST_R, ST_LD = 0, 1, 2, 3, 4, 260, 324, 388       # ZSG_GC_STAT_* of include/zsg.h
LEVELS = {"1x1": [(1, 1)], "3x3": [(3, 3)], "5x7": [(5, 7)], "chunk-1": [(7, 9)], "chunk": [(8, 8)], "chunk+1": [(5, 13)],
          "mixed": [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]}
SIZES_300 = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3)]
CASES = [(k, q) for k in LEVELS for q in (1, 3)] + [("pyramid300", 2)]
SHAPES = {"key.weight": (1, N), "fc1.weight": (M, N), "fc1.bias": (M,), "ln.weight": (M,), "ln.bias": (M,), "fc2.weight": (N, M), "fc2.bias": (N,)}
GRADS = ("dkey", "dW1", "db1", "dlnw", "dlnb", "dW2", "db2")
CANARY = 1024
MARK = 12345.0
NAN = float("nan")
assert LEVELS["chunk-1"][0][0] * LEVELS["chunk-1"][0][1] == CHUNK - 1 and LEVELS["chunk+1"][0][0] * LEVELS["chunk+1"][0][1] == CHUNK + 1


def sizes_of(geom):
    return SIZES_300 if geom == "pyramid300" else LEVELS[geom]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as L
    return L


class Guarded:
    """a device buffer of n elements between two canary runs, pre-filled with `fill`"""

    def __init__(self, n, dtype=torch.float32, fill=NAN):
        self.buf = torch.full((2 * CANARY + n,), fill, dtype=dtype, device="cuda")
        self.buf[:CANARY] = MARK
        self.buf[-CANARY:] = MARK
        self.view = self.buf[CANARY:CANARY + n]

    def intact(self):
        return bool((self.buf[:CANARY] == MARK).all()) and bool((self.buf[-CANARY:] == MARK).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def hw_of(sizes):
    return torch.tensor([v for s_ in sizes for v in s_], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def operands(geom, Q, seed=0):
    """fp32 operands: x post-ReLU like h1, g, the seven parameters (drawn, fc2 included)"""
    sizes = sizes_of(geom)
    g = torch.Generator().manual_seed(1000 * seed + 7 * Q + len(geom))
    x = [torch.relu(torch.randn(Q, h * w, N, generator=g)) for h, w in sizes]
    gy = [torch.randn(Q, h * w, N, generator=g) for h, w in sizes]
    par = {n: torch.randn(*s, generator=g) * (1.0 if n in ("ln.weight",) else 0.1) for n, s in SHAPES.items()}
    return dict(x=x, g=gy, par=par)


def reference(d, dtype):
    """(y levels, dx levels, the seven gradients by GRADS' names, c [nlev][Q][N]) of gc_ref in `dtype` on the CPU"""
    x = [t.detach().clone().to(dtype).requires_grad_(True) for t in d["x"]]               # (fresh leaves: the cached operands stay as drawn)
    par = [d["par"][n].detach().clone().to(dtype).requires_grad_(True) for n in GR.NAMES]
    ys, cs = zip(*[GR.gc_rows(t, *par) for t in x])
    loss = sum((y * g.to(dtype)).sum() for y, g in zip(ys, d["g"]))
    loss.backward()
    return ([y.detach() for y in ys], [t.grad for t in x], {k: p.grad for k, p in zip(GRADS, par)}, [c.detach() for c in cs])


@functools.lru_cache(maxsize=None)
def truth_and_yardstick(geom, Q):
    """computed once per geometry, shared by the tests and left unchanged"""
    d = operands(geom, Q)
    return reference(d, torch.float64), reference(d, torch.float32)


def pack(levels):
    return torch.cat([t.reshape(-1) for t in levels]).cuda()


def unpack(flat, Q, sizes, C=N):
    out, p0 = [], 0
    for h, w in sizes:
        out.append(flat[Q * p0 * C:Q * (p0 + h * w) * C].view(Q, h * w, C))
        p0 += h * w
    return out


def dev_params(par):
    return {n: par[n].reshape(-1).contiguous().cuda() for n in GR.NAMES}


def run_forward(L, d, sizes, Q, train=True, fill=NAN):
    """(y flat, s flat or None, stat [nlev * Q, ST_LD] or None)"""
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    nws = int(L.lib.zsg_head_gc_fwd_ws_bytes(Q, len(sizes), hw.data_ptr(), N))
    assert nws > 0
    ws = Guarded((nws + 3) // 4, fill=fill)
    y, s, stat = Guarded(Q * P * N, fill=fill), Guarded(Q * P, fill=fill), Guarded(Q * len(sizes) * ST_LD, fill=fill)
    xd, p = pack(d["x"]), dev_params(d["par"])
    rc = L.lib.zsg_head_gc_fwd(xd.data_ptr(), *[p[n].data_ptr() for n in GR.NAMES], Q, len(sizes), hw.data_ptr(), N, y.view.data_ptr(),
                               s.view.data_ptr() if train else None, stat.view.data_ptr() if train else None, ws.view.data_ptr(), nws, L.stream_ptr())
    L.check(rc, "head_gc_fwd")
    torch.cuda.synchronize()
    assert y.intact() and s.intact() and stat.intact() and ws.intact(), "a canary around y / s / stat / ws was overwritten"
    if not train:
        assert bool(torch.isnan(s.view).all()) and bool(torch.isnan(stat.view).all()), "the eval forward saves nothing"
        return y.view.clone().cpu(), None, None
    return y.view.clone().cpu(), s.view.clone(), stat.view.clone()


def run_backward(L, d, s, stat, sizes, Q, want_dx=True, want=GRADS, accumulate=0, fill=NAN):
    """(dx flat or None, {name: gradient}) — only the outputs asked for are passed"""
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    nws = int(L.lib.zsg_head_gc_bwd_ws_bytes(Q, len(sizes), hw.data_ptr(), N))
    assert nws > 0
    ws = Guarded((nws + 7) // 8, torch.float64, fill)
    dx = Guarded(Q * P * N, fill=fill)
    numel = dict(zip(GRADS, (N, M * N, M, M, M, N * M, N)))
    outs = {k: Guarded(numel[k], fill=(1.0 if accumulate else fill)) for k in GRADS}
    gd, xd, p = pack(d["g"]), pack(d["x"]), dev_params(d["par"])
    rc = L.lib.zsg_head_gc_bwd(gd.data_ptr(), xd.data_ptr(), s.data_ptr(), stat.data_ptr(), p["key.weight"].data_ptr(), p["fc1.weight"].data_ptr(),
                               p["ln.weight"].data_ptr(), p["fc2.weight"].data_ptr(), Q, len(sizes), hw.data_ptr(), N,
                               dx.view.data_ptr() if want_dx else None, *[outs[k].view.data_ptr() if k in want else None for k in GRADS],
                               accumulate, ws.view.data_ptr(), nws, L.stream_ptr())
    L.check(rc, "head_gc_bwd")
    torch.cuda.synchronize()
    assert dx.intact() and ws.intact() and all(o.intact() for o in outs.values()), "a canary was overwritten"
    if not want_dx:
        assert bool(torch.isnan(dx.view).all())
    for k in GRADS:
        if k not in want:
            assert bool((outs[k].view == 1.0).all() if accumulate else torch.isnan(outs[k].view).all()), k + " was written without being asked for"
    return (dx.view.clone().cpu() if want_dx else None), {k: outs[k].view.clone().cpu() for k in want}


def err(got, want64):
    return float((got.double().reshape(-1) - want64.reshape(-1)).abs().max())


@pytest.mark.parametrize("geom,Q", CASES)
def test_random_inputs_against_the_reference(L, geom, Q):
    sizes = sizes_of(geom)
    d = operands(geom, Q)
    (y64, dx64, g64, c64), (y32, dx32, g32, _) = truth_and_yardstick(geom, Q)
    y, s, stat = run_forward(L, d, sizes, Q)
    ye, _, _ = run_forward(L, d, sizes, Q, train=False)
    assert torch.equal(bits(y), bits(ye)), "the eval forward carries the training forward's bits"
    dx, grads = run_backward(L, d, s, stat, sizes, Q)
    cat = lambda lv: torch.cat([t.reshape(-1) for t in lv])
    rows = [("y", y, cat(y64), cat(y32)), ("dx", dx, cat(dx64), cat(dx32))] + [(k, grads[k], g64[k], g32[k]) for k in GRADS]
    report = []
    for name, got, want, yard in rows:
        e_gpu, e_cpu = err(got, want), err(yard, want)
        report.append((name, e_gpu, e_cpu, 4 * e_cpu))
        print(f"gc parity {geom} Q={Q} {name}: gpu {e_gpu:.3e} cpu_fp32 {e_cpu:.3e} bound {4 * e_cpu:.3e} scale {float(want.abs().max()):.3e}")
    for name, e_gpu, e_cpu, bound in report:
        assert e_gpu <= bound, (geom, Q, name, e_gpu, e_cpu)
    # the saved context vector against the truth's, at the yardstick-free bound of an fp32 softmax-weighted mean
    c = stat.cpu().view(len(sizes), Q, ST_LD)[:, :, ST_C:ST_C + N]
    for i in range(len(sizes)):
        assert err(c[i], c64[i]) <= 1e-5 * max(1.0, float(c64[i].abs().max()))
    # accumulate = 1 adds the same value to what the buffer holds
    _, acc = run_backward(L, d, s, stat, sizes, Q, want_dx=False, accumulate=1)
    for k in GRADS:
        assert torch.equal(bits(acc[k]), bits(1.0 + grads[k])), k


@pytest.mark.parametrize("geom,Q", CASES)
def test_zero_last_layer_is_the_identity(L, geom, Q):
    sizes = sizes_of(geom)
    d0 = operands(geom, Q)
    d = dict(d0, par=dict(d0["par"], **{"fc2.weight": torch.zeros(N, M), "fc2.bias": torch.zeros(N)}))
    y, s, stat = run_forward(L, d, sizes, Q)
    assert torch.equal(y, pack(d["x"]).cpu()), "y = x"
    dx, grads = run_backward(L, d, s, stat, sizes, Q)
    assert torch.equal(dx, pack(d["g"]).cpu()), "dx = g"
    (_, _, g64, _), (_, _, g32, _) = reference(d, torch.float64), reference(d, torch.float32)
    for k in ("dW2", "db2"):
        assert err(grads[k], g64[k]) <= 4 * err(g32[k], g64[k]), k
        assert grads[k].any()
    for k in ("dkey", "dW1", "db1", "dlnw", "dlnb"):
        assert not grads[k].any(), k + ": nothing reaches the layers in front of a zero fc2.weight"


@pytest.mark.parametrize("geom,Q", [("5x7", 3), ("chunk+1", 1), ("mixed", 3)])
def test_zero_key_pools_the_row_mean(L, geom, Q):
    sizes = sizes_of(geom)
    d0 = operands(geom, Q)
    d = dict(d0, par=dict(d0["par"], **{"key.weight": torch.zeros(1, N)}))
    _, s, stat = run_forward(L, d, sizes, Q)
    assert not s.any()
    st = stat.cpu().view(len(sizes), Q, ST_LD)
    for i, (h, w) in enumerate(sizes):
        P = h * w
        x = d["x"][i].double()
        assert bool((st[i, :, ST_DEN] == P).all()) and not st[i, :, ST_MAX].any()
        bound = (P + 1) * 2.0 ** -24 * float(x.abs().max())
        assert err(st[i, :, ST_C:ST_C + N], x.mean(dim=1)) <= bound, (geom, i)


@pytest.mark.parametrize("geom,Q", [("chunk+1", 3), ("mixed", 1)])
def test_large_logits_stay_finite(L, geom, Q):
    sizes = sizes_of(geom)
    d0 = operands(geom, Q)
    k = d0["par"]["key.weight"]
    top = max(float((x @ k.reshape(-1)).abs().max()) for x in d0["x"])
    d = dict(d0, par=dict(d0["par"], **{"key.weight": k * (80.0 / top)}))
    assert abs(max(float((x @ d["par"]["key.weight"].reshape(-1)).abs().max()) for x in d["x"]) - 80.0) < 1e-2
    y, s, stat = run_forward(L, d, sizes, Q)
    dx, grads = run_backward(L, d, s, stat, sizes, Q)
    assert float(s.abs().max()) > 79.0
    for name, t in [("y", y), ("s", s), ("stat", stat), ("dx", dx)] + list(grads.items()):
        assert bool(torch.isfinite(t).all()), name
    y64, dx64, g64, _ = reference(d, torch.float64)
    cat = lambda lv: torch.cat([t.reshape(-1) for t in lv])
    assert err(y, cat(y64)) <= 1e-4 * float(cat(y64).abs().max()) and err(dx, cat(dx64)) <= 1e-4 * float(cat(dx64).abs().max())


@pytest.mark.parametrize("geom,Q", [("chunk+1", 3), ("mixed", 3), ("pyramid300", 2)])
def test_two_runs_give_the_same_bits(L, geom, Q):
    sizes = sizes_of(geom)
    d = operands(geom, Q)
    a = run_forward(L, d, sizes, Q, fill=NAN)
    b = run_forward(L, d, sizes, Q, fill=-7.0)
    for u, v in zip(a, b):
        assert torch.equal(bits(u), bits(v))
    ga = run_backward(L, d, a[1], a[2], sizes, Q, fill=NAN)
    gb = run_backward(L, d, a[1], a[2], sizes, Q, fill=-7.0)
    assert torch.equal(bits(ga[0]), bits(gb[0]))
    for k in GRADS:
        assert torch.equal(bits(ga[1][k]), bits(gb[1][k])), k


def test_frozen_outputs_are_left_alone(L):
    """NULL outputs are skipped and the others keep their bits: only-gc (no dx), all-but-gc (dx alone), one gradient at a time"""
    geom, Q = "mixed", 3
    sizes = sizes_of(geom)
    d = operands(geom, Q)
    _, s, stat = run_forward(L, d, sizes, Q)
    dx, grads = run_backward(L, d, s, stat, sizes, Q)
    _, only = run_backward(L, d, s, stat, sizes, Q, want_dx=False)
    assert all(torch.equal(bits(only[k]), bits(grads[k])) for k in GRADS)
    dx2, none = run_backward(L, d, s, stat, sizes, Q, want=())
    assert torch.equal(bits(dx2), bits(dx)) and not none
    for k in GRADS:
        _, one = run_backward(L, d, s, stat, sizes, Q, want_dx=False, want=(k,))
        assert torch.equal(bits(one[k]), bits(grads[k])), k


def test_bad_arguments_are_refused_by_name(L):
    geom, Q = "3x3", 1
    sizes = sizes_of(geom)
    d = operands(geom, Q)
    P = 9
    hw = hw_of(sizes)
    xd, gd, p = pack(d["x"]), pack(d["g"]), dev_params(d["par"])
    y, s, stat, dx = Guarded(Q * P * N), Guarded(Q * P), Guarded(Q * ST_LD), Guarded(Q * P * N)
    ws = Guarded(1 << 16, torch.float64)
    nws = ws.view.numel() * 8
    grads = [Guarded(n) for n in (N, M * N, M, M, M, N * M, N)]
    many = hw_of([(1, 1)] * 9)
    empty = hw_of([(3, 0)])                 # (kept alive: the call reads the tensor's memory)

    def fwd(**kw):
        a = dict(x=xd.data_ptr(), key=p["key.weight"].data_ptr(), W1=p["fc1.weight"].data_ptr(), b1=p["fc1.bias"].data_ptr(),
                 lnw=p["ln.weight"].data_ptr(), lnb=p["ln.bias"].data_ptr(), W2=p["fc2.weight"].data_ptr(), b2=p["fc2.bias"].data_ptr(), Q=Q,
                 nlev=1, hw=hw.data_ptr(), N=N, y=y.view.data_ptr(), s=s.view.data_ptr(), stat=stat.view.data_ptr(), ws=ws.view.data_ptr(),
                 ws_bytes=nws)
        a.update(kw)
        return L.lib.zsg_head_gc_fwd(*a.values(), L.stream_ptr())

    def bwd(**kw):
        a = dict(g=gd.data_ptr(), x=xd.data_ptr(), s=s.view.data_ptr(), stat=stat.view.data_ptr(), key=p["key.weight"].data_ptr(),
                 W1=p["fc1.weight"].data_ptr(), lnw=p["ln.weight"].data_ptr(), W2=p["fc2.weight"].data_ptr(), Q=Q, nlev=1, hw=hw.data_ptr(), N=N,
                 dx=dx.view.data_ptr(), dkey=grads[0].view.data_ptr(), dW1=grads[1].view.data_ptr(), db1=grads[2].view.data_ptr(),
                 dlnw=grads[3].view.data_ptr(), dlnb=grads[4].view.data_ptr(), dW2=grads[5].view.data_ptr(), db2=grads[6].view.data_ptr(),
                 accumulate=0, ws=ws.view.data_ptr(), ws_bytes=nws)
        a.update(kw)
        return L.lib.zsg_head_gc_bwd(*a.values(), L.stream_ptr())

    def refused(rc, word):
        msg = L.lib.zsg_last_error().decode()
        assert rc == -1 and word in msg, (rc, word, msg)

    for name in ("x", "key", "W1", "b1", "lnw", "lnb", "W2", "b2", "y", "ws", "hw"):
        refused(fwd(**{name: None}), name + " is NULL")
    for name in ("g", "x", "s", "stat", "key", "W1", "lnw", "W2", "ws", "hw"):
        refused(bwd(**{name: None}), name + " is NULL")
    for fn in (fwd, bwd):
        refused(fn(N=128), "N = 128")
        refused(fn(N=512), "N = 512")
        refused(fn(nlev=0), "nlev = 0")
        refused(fn(nlev=9, hw=many.data_ptr()), "nlev = 9")
        refused(fn(Q=0), "Q = 0")
        refused(fn(ws_bytes=64), "ws_bytes")
        refused(fn(x=xd.data_ptr() + 4), "x is not 16-byte aligned")
        refused(fn(hw=empty.data_ptr()), "hw: level 0 is empty")
    refused(fwd(s=None), "s and stat")
    refused(fwd(stat=None), "s and stat")
    refused(bwd(dx=None, dkey=None, dW1=None, db1=None, dlnw=None, dlnb=None, dW2=None, db2=None), "no output")
    torch.cuda.synchronize()
    for b in [y, s, stat, dx, ws] + grads:
        assert b.intact() and bool(torch.isnan(b.view).all()), "a refused call wrote nothing"

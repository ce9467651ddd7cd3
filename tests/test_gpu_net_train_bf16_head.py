"""train_dtype = "bf16_head" on the network: ZSGNet.train_precision / cfg train_dtype, the training plan whose pyramid and head convolutions
run on zsg_conv_igemm_bf16 (forward) and zsg_conv_igemm_bf16_m (data gradients).  ResNet-18, 128 px, B = 2,
O.seeded_state_dict("resnet18", 1), O.synthetic_batch(2, 128, 128, seed=3), fixed h0 / c0 — the set-up of tests/test_gpu_net_wgrad_bf16.py,
under ZSG_DETERMINISTIC=1 (no atomic split-K in the fp32 launches: two fp32 steps give the same bits).

Exact part: everything in front of the pyramid is untouched, so every BatchNorm's running statistics, the encoder activations feeding
P3_1 / P4_1 / P5_1 and the LSTM's output are bit-equal to the fp32 net's.

Layer-local part (the rigorous one): every launch on the new path is in plan._b16_log with its operands; each is recomputed on the host
from the GPU's OWN operand bits and the current parameters — both rounded to bf16 (torch's round-to-nearest-even), fp64 sums, bias /
add_src / ReLU / mask in kernel order — and compared under the bound derived in tests/test_gpu_conv_bf16.py,
    |out - ref| <= (K + 4) * 2^-23 * (S + |bias| + |add_src|),   K = taps * C, S the same sum of absolute values.
Every launch is compared as the STEP left it — its dx was written behind that step's pack launch — with one exception: conv0's data
gradient writes the gradient of the packed pyramid, and the backward of P8's pooling and of relu(P6) later add to two of its levels, so
after the step it no longer holds the launch's own result.  That one launch (REPLAY) is replayed once, alone, on its unchanged operands
before dx is read, and it is checked last, because its replay takes those additions out of P7_2's dy.  Entries with add_src (the data gradients of P4_2 / P5_2, whose dx already holds the top-down branch) are skipped:
their incoming dx is overwritten.  No end-to-end emulation is used as a reference: a CPU emulation of this set-up disagrees with itself
by 4e-2 in the flat gradient between fp32 and fp64, because tiny differences flip bf16 roundings.

Rounded part against the fp32 plan: each bound is 4 x the value measured on an MI355X, rounded up to one digit, and may not exceed the
caps below (profiles/train_bf16_head_parity_measured.txt).  Measured: box 7.858e-3, att 5.985e-3, loss 1.518e-3 (30.346716 -> 30.300661),
flat-gradient L2 6.111e-2, 1 - cosine 1.848e-3.  A CPU emulation (fp64, operands rounded in the pyramid and the heads only) gives
outputs 5.6-7.4e-3, loss 1.3e-3, flat L2 4.7-6.3e-2, cosine 0.998, per parameter up to 1.6e-1.  Per-parameter distances are printed,
not bounded."""
import ctypes as C
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

CAP_BOX, CAP_ATT, CAP_L2, CAP_COS = 5e-2, 6e-2, 0.3, 0.98
MEASURED = dict(box=7.858e-3, att=5.985e-3, loss=1.518e-3, l2=6.111e-2, one_minus_cos=1.848e-3)
BOUND_BOX = 4e-2          # 4 x 7.858e-3 = 3.14e-2, rounded up to one digit
BOUND_ATT = 3e-2          # 4 x 5.985e-3 = 2.39e-2
BOUND_LOSS = 7e-3         # 4 x 1.518e-3 = 6.07e-3
BOUND_L2 = 0.3            # 4 x 6.111e-2 = 2.44e-1
BOUND_COS = 1 - 8e-3      # 1 - 4 x 1.848e-3 = 1 - 7.39e-3
assert BOUND_BOX <= CAP_BOX and BOUND_ATT <= CAP_ATT and BOUND_L2 <= CAP_L2 and BOUND_COS >= CAP_COS

ENC = "backbone.encoder."
FPN = "backbone.fpn."
HEAD = "att_reg_box."
FWD_LAYERS = [FPN + n for n in ("P3_1", "P4_1", "P5_1", "P3_2", "P4_2", "P5_2", "P6", "P7_2")] + [HEAD + "0.0"] + [f"{HEAD}{i}.0" for i in range(1, 5)] + [HEAD + "5"]
DGRAD_LAYERS = [n for n in FWD_LAYERS if n[len(FPN):] not in ("P3_1", "P4_1", "P5_1", "P6")]       # (those four land in a BatchNorm output)
REPLAY = {"dgrad:" + HEAD + "0.0"}       # the data gradients whose dx a later launch of the backward adds to (see the docstring)
CONVS = ("zsg_conv_igemm", "zsg_conv_wino")
WG = {"zsg_conv_wgrad", "zsg_conv_wgrad_wino", "zsg_conv_wgrad_wino_batched", "zsg_conv_wgrad_bf16"}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, loss, mdl, optim, synth
    return dict(L=_lib, config=config, loss=loss, mdl=mdl, optim=optim, synth=synth)


@pytest.fixture(scope="module", autouse=True)
def deterministic(Z):
    L = Z["L"]
    old = os.environ.get("ZSG_DETERMINISTIC")
    os.environ["ZSG_DETERMINISTIC"] = "1"
    L.lib.zsg_set_deterministic(1)
    yield
    if old is None:
        os.environ.pop("ZSG_DETERMINISTIC", None)
    else:
        os.environ["ZSG_DETERMINISTIC"] = old
    L.lib.zsg_set_deterministic(1 if old == "1" else 0)


def build(Z, **flags):
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", **flags)
    net = Z["mdl"].get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 1))
    return cfg, net.to("cuda")


def batch(B=2):
    bt = O.synthetic_batch(B, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)
    return inp


def shared_batch(Z):
    bt = Z["synth"].synthetic_shared_batch(2, 4, 128, 128, seed=5)
    bt["img_idx"] = torch.tensor([1, 0, 0, 1])
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.zeros(2, 4, 128), torch.zeros(2, 4, 128)
    return inp


def loss_fn(Z, cfg):
    r, s = Z["config"].ratios_scales(cfg)
    return Z["loss"].get_default_loss(r, s, cfg)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def train_plan(net):
    ks = [k for k in net._plans if k[-1]]
    assert len(ks) == 1, ks
    return net._plans[ks[0]]


def listing(prog):
    return [(lane, fn.__name__, what) for (fn, _, what), lane in zip(prog.calls, prog.lanes)]


def step(Z, cfg, net, inp):
    """zero_grad + forward + loss + backward; returns (att_bbx_out, loss terms, the flat gradient) on the CPU"""
    net.train()
    net.store.grad.zero_()
    out = net(inp)
    ls = loss_fn(Z, cfg)(out, inp)
    ls["loss"].mean().backward()
    torch.cuda.synchronize()
    return out["att_bbx_out"].detach().cpu().clone(), {k: v.detach().cpu().clone() for k, v in ls.items() if torch.is_tensor(v)}, net.store.grad.detach().cpu().clone()


def grad_of(net, flat, name):
    e = net.store.entries[name]
    return flat[e.offset:e.offset + e.size]


# ---- the layer-local reference ----------------------------------------------------------------------------------------------------------
def level_view(act, buf, i, Cc):
    """[B, H, W, Cc] view of level i of an activation laid out as `act` says, in the CPU copy `buf` of its buffer"""
    lv = act.levels[i]
    return torch.as_strided(buf, (act.B, lv.H, lv.W, Cc), (lv.bstride, lv.W * act.ld, act.ld, 1), lv.off)


def conv_out(n, k, s, p):
    return (n + 2 * p - (k - 1) - 1) // s + 1


def conv_ref(src, w, k, s, p, Ho, Wo):
    B, H, W, Cc = src.shape
    pad = torch.zeros(B, H + 2 * p, W + 2 * p, Cc, dtype=src.dtype)
    pad[:, p:p + H, p:p + W] = src
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=src.dtype)
    for ty in range(k):
        for tx in range(k):
            win = pad[:, ty: ty + (Ho - 1) * s + 1: s, tx: tx + (Wo - 1) * s + 1: s]
            out += torch.matmul(win.reshape(-1, Cc), w[:, ty, tx].t()).view(B, Ho, Wo, -1)
    return out


def dgrad_ref(dy, w, H, W, k, s, p):
    B, Ho, Wo, co = dy.shape
    buf = torch.zeros(B, H + 2 * p, W + 2 * p, w.shape[3], dtype=dy.dtype)
    for ty in range(k):
        for tx in range(k):
            buf[:, ty: ty + (Ho - 1) * s + 1: s, tx: tx + (Wo - 1) * s + 1: s] += torch.matmul(dy.reshape(-1, co), w[:, ty, tx]).view(B, Ho, Wo, -1)
    return buf[:, p:p + H, p:p + W].contiguous()


def local_check(net, plan, e, flat, out5=None):
    """recompute the logged launch `e` on the host from the GPU's own operand bits and the parameters in `flat` (a CPU copy of the flat
    weight buffer); returns the largest |out - ref| / bound over its elements (<= 1 passes)"""
    L = net.convs[e["pname"][:-len(".weight")]]
    assert L.dil == 1
    ent = net.store.entries[e["pname"]]
    w = flat[ent.offset:ent.offset + L.cout * L.k * L.k * L.cpad].view(L.cout, L.k, L.k, L.cpad)
    d = e["d"]
    src_b = e["src"].buf.detach().cpu()
    worst = 0.0
    if e["kind"] == "fwd":
        wc0, Cc = e["window"]
        assert (d.C, d.N) == (Cc, L.cout)
        out_b = out5.reshape(-1) if (out5 is not None and e["out"] is plan.out5) else e["out"].buf.detach().cpu()
        add_b = e["add"].buf.detach().cpu() if e["add"] is not None else None
        bias = None
        if L.bias and not e["what"].endswith(".feat"):                # (the shared-image form leaves conv0's raw accumulator: no bias, no ReLU)
            be = net.store.entries[L.name + ".bias"]
            bias = flat[be.offset:be.offset + L.cout].double()
        wb = w[..., wc0:wc0 + Cc].to(torch.bfloat16).double()
        for i, lo in enumerate(e["out"].levels):
            x = level_view(e["src"], src_b, i, Cc).to(torch.bfloat16).double()
            r, S = conv_ref(x, wb, L.k, L.stride, L.pad, lo.H, lo.W), conv_ref(x.abs(), wb.abs(), L.k, L.stride, L.pad, lo.H, lo.W)
            if bias is not None:
                r, S = r + bias, S + bias.abs()
            if add_b is not None:
                a = level_view(e["add"], add_b, i, L.cout).double()
                r, S = r + a, S + a.abs()
            if d.relu:
                r = r.clamp(min=0)
            got = level_view(e["out"], out_b, i, L.cout).double()
            assert bool(torch.isfinite(got).all())
            bound = (L.k * L.k * Cc + 4) * 2.0 ** -23 * S
            worst = max(worst, float(((got - r).abs() / bound.clamp(min=1e-300)).max()))
        return worst
    row0, n = e["window"]
    assert e["add"] is None and (d.N, d.C) == (n, e["src"].ld)
    fn, args, _ = plan.bwd.calls[e["idx"]]
    assert fn.__name__ == "zsg_conv_igemm_bf16_m"
    if e["what"] in REPLAY:
        # the launch alone, once more, on its unchanged operands: dx then holds this launch's own result
        assert fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
    out_b = e["out"].buf.detach().cpu()
    mask_b = e["mask"].buf.detach().cpu() if e["mask"] is not None else None
    wb = w[..., row0:row0 + n].to(torch.bfloat16).double()
    for i, lx in enumerate(e["out"].levels):
        dy = level_view(e["src"], src_b, i, L.cout).to(torch.bfloat16).double()
        r, S = dgrad_ref(dy, wb, lx.H, lx.W, L.k, L.stride, L.pad), dgrad_ref(dy.abs(), wb.abs(), lx.H, lx.W, L.k, L.stride, L.pad)
        got = level_view(e["out"], out_b, i, n).double()
        assert bool(torch.isfinite(got).all())
        if mask_b is not None:
            on = level_view(e["mask"], mask_b, i, n) > 0
            assert bool((got[~on] == 0).all()), e["what"] + ": a masked element is not zero"
            r = torch.where(on, r, torch.zeros_like(r))
        bound = (L.k * L.k * e["src"].ld + 4) * 2.0 ** -23 * S
        worst = max(worst, float(((got - r).abs() / bound.clamp(min=1e-300)).max()))
    return worst


def check_all(net, plan, out5, want_skipped):
    flat = net.store.flat.detach().cpu()
    skipped, res = [], {}
    for e in sorted(plan._b16_log, key=lambda e: e["what"] in REPLAY):          # (stable: the replayed launch goes last)
        if e["kind"] == "dgrad" and e["add"] is not None:
            skipped.append(e["what"])
            continue
        res[(e["kind"], e["what"])] = local_check(net, plan, e, flat, out5)
    assert sorted(skipped) == sorted(want_skipped), skipped
    for k, v in sorted(res.items()):
        print(f"bf16_head layer-local {k[0]:5s} {k[1]:36s} max |out - ref| / bound = {v:.4f}")
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad
    return res


@pytest.fixture(scope="module")
def ref(Z, deterministic):
    """one step of the fp32 net and of the bf16_head net on the module's set-up (computed once, never modified)"""
    inp = batch()
    cfg, net32 = build(Z)
    o32, l32, g32 = step(Z, cfg, net32, inp)
    cfg16, net16 = build(Z, train_dtype="bf16_head")
    assert net16._train_dtype == "bf16_head"
    o16, l16, g16 = step(Z, cfg16, net16, inp)
    return dict(inp=inp, cfg=cfg, cfg16=cfg16, net32=net32, net16=net16, o32=o32, l32=l32, g32=g32, o16=o16, l16=l16, g16=g16)


def swap(l32, names, prefix, new_fn):
    """the fp32 listing with the convolution launches of `names` replaced by the bf16 entry's"""
    whats = {prefix + n for n in names}
    out = []
    for lane, fn, what in l32:
        if what in whats and fn in CONVS:
            out.append((lane, new_fn, what + "+bf16"))
        else:
            out.append((lane, fn, what))
    return out


def test_programs(Z, ref):
    p32, p16 = train_plan(ref["net32"]), train_plan(ref["net16"])
    (key,) = [k for k in ref["net16"]._plans if k[-1]]
    assert ("train", "bf16_head") in key and not any(isinstance(e, tuple) and e and e[0] == "train" for e in list(ref["net32"]._plans)[0])
    f32, f16, b32, b16 = listing(p32.fwd), listing(p16.fwd), listing(p32.bwd), listing(p16.bwd)
    assert not any("bf16" in n or w.endswith("+bf16") for prog in (f32, b32, listing(p32.prep), listing(p32.prep_u)) for _, n, w in prog)
    assert not p32._b16_log
    # forward: differs exactly at the eligible layers (the same lanes, the same places); none of them is a Winograd launch any more
    assert f16 == swap(f32, FWD_LAYERS, "", "zsg_conv_igemm_bf16")
    assert sorted(w for _, n, w in f16 if n == "zsg_conv_igemm_bf16") == sorted(n + "+bf16" for n in FWD_LAYERS)
    assert not any(n.startswith("zsg_conv_wino") and w.startswith((FPN, HEAD)) for _, n, w in f16)
    assert all(not w.startswith(ENC) for _, n, w in f16 if "bf16" in n)
    # ONE pack launch per forward (with the weight-only work on the side stream), ONE per backward (behind the transpose)
    pu, pp = listing(p16.prep_u), listing(p16.prep)
    assert [n for _, n, _ in pu].count("zsg_pack_w_bf16_batched") == 1 and not any(n == "zsg_pack_w_bf16_batched" for _, n, _ in f16)
    assert len(p16.pack_jobs) == len(FWD_LAYERS)
    names = [n for _, n, _ in pp]
    assert names.count("zsg_pack_w_bf16_batched") == 1 and names.index("zsg_pack_w_bf16_batched") == names.index("zsg_transpose_w_batched") + 1
    assert len(p16.dpack_jobs) == len(DGRAD_LAYERS)
    first = min(e["idx"] for e in p16._b16_log if e["kind"] == "fwd")
    assert p16._wait_idx <= first, "the main stream waits for the pack launch in front of the first reader"
    # backward: differs exactly at the eligible data gradients; the laterals' and P6's are the fp32 plan's launches
    assert b16 == swap(b32, DGRAD_LAYERS, "dgrad:", "zsg_conv_igemm_bf16_m")
    assert sorted(w for _, n, w in b16 if n == "zsg_conv_igemm_bf16_m") == sorted("dgrad:" + n + "+bf16" for n in DGRAD_LAYERS)
    for nm in ("P3_1", "P4_1", "P5_1", "P6"):
        a = [(n, w) for _, n, w in b32 if w.startswith("dgrad:" + FPN + nm)]
        assert a and a == [(n, w) for _, n, w in b16 if w.startswith("dgrad:" + FPN + nm)] and all("bf16" not in n for n, _ in a)
    # every weight-gradient launch is the fp32 plan's
    assert [(l, n, w) for l, n, w in b32 if n in WG] == [(l, n, w) for l, n, w in b16 if n in WG]
    assert set(p16.grad_ready) == set(p32.grad_ready)
    # the log: one entry per launch, pointing at it
    assert [(e["kind"], e["what"]) for e in p16._b16_log if e["kind"] == "fwd"] and len(p16._b16_log) == len(FWD_LAYERS) + len(DGRAD_LAYERS)
    for e in p16._b16_log:
        prog = p16.fwd if e["kind"] == "fwd" else p16.bwd
        fn, _, what = prog.calls[e["idx"]]
        assert fn.__name__ == ("zsg_conv_igemm_bf16" if e["kind"] == "fwd" else "zsg_conv_igemm_bf16_m") and what == e["what"] + "+bf16"
        assert e["pname"] in ref["net16"].store.entries and e["src"] is not None and e["out"] is not None
    masks = {e["what"]: e["mask"] is not None for e in p16._b16_log if e["kind"] == "dgrad"}
    assert masks == {"dgrad:" + n: (n.startswith(HEAD) and not n.endswith("0.0")) for n in DGRAD_LAYERS}, "the head's ReLU masks"


def test_programs_with_bf16_weight_gradients_and_a_net_that_never_saw_the_key(Z, ref):
    inp = ref["inp"]
    cfgw, netw = build(Z, wgrad_dtype="bf16")
    step(Z, cfgw, netw, inp)
    cfgb, netb = build(Z, wgrad_dtype="bf16", train_dtype="bf16_head")
    step(Z, cfgb, netb, inp)
    (key,) = [k for k in netb._plans if k[-1]]
    assert ("train", "bf16_head") in key and ("wgrad", "bf16") in key
    bw, bb = listing(train_plan(netw).bwd), listing(train_plan(netb).bwd)
    assert [(l, n, w) for l, n, w in bw if n in WG] == [(l, n, w) for l, n, w in bb if n in WG]
    assert bb == swap(bw, DGRAD_LAYERS, "dgrad:", "zsg_conv_igemm_bf16_m")
    assert listing(train_plan(netb).fwd) == listing(train_plan(ref["net16"]).fwd)
    # a net that never heard of the switch lowers the fp32 net's programs and gives its bits
    cfg = Z["config"].get_cfg(resnet_arch="resnet18")
    cfg.pop("train_dtype")
    net0 = Z["mdl"].get_default_net(9, cfg)
    net0.load_state_dict(O.seeded_state_dict("resnet18", 1))
    net0.to("cuda")
    o0, _, g0 = step(Z, cfg, net0, inp)
    p0, p32 = train_plan(net0), train_plan(ref["net32"])
    assert listing(p0.bwd) == listing(p32.bwd) and listing(p0.fwd) == listing(p32.fwd)
    assert listing(p0.prep) == listing(p32.prep) and listing(p0.prep_u) == listing(p32.prep_u)
    assert list(net0._plans) == list(ref["net32"]._plans)
    assert torch.equal(bits(g0), bits(ref["g32"])) and torch.equal(bits(o0), bits(ref["o32"]))


def test_exact_part(Z, ref):
    n32, n16 = ref["net32"], ref["net16"]
    assert torch.equal(bits(n32._rmv), bits(n16._rmv)), "BatchNorm running statistics"
    assert torch.equal(n32._nbt.cpu(), n16._nbt.cpu())
    p32, p16 = train_plan(n32), train_plan(n16)
    lat = {e["what"]: e["src"] for e in p16._b16_log if e["kind"] == "fwd" and e["what"][len(FPN):] in ("P3_1", "P4_1", "P5_1")}
    assert len(lat) == 3
    for what, a in lat.items():
        assert a.name in p32.acts and torch.equal(bits(a.buf), bits(p32.acts[a.name].buf)), f"encoder activation feeding {what}"
        assert float(a.buf.abs().max()) > 0
    assert torch.equal(bits(p16.acts["we"].buf), bits(p32.acts["we"].buf)), "the LSTM's output"


def test_layer_local(Z, ref):
    """every forward launch and every data gradient without add_src of the step in `ref`, from the GPU's own operand bits"""
    net, plan = ref["net16"], train_plan(ref["net16"])
    res = check_all(net, plan, ref["o16"], ["dgrad:" + FPN + "P4_2", "dgrad:" + FPN + "P5_2"])
    assert len(res) == len(FWD_LAYERS) + len(DGRAD_LAYERS) - 2
    assert len([e for e in plan._b16_log if e["kind"] == "dgrad"]) == 10


def test_rounded_part_against_the_fp32_plan(Z, ref):
    o32, o16, g32, g16 = ref["o32"].double(), ref["o16"].double(), ref["g32"].double(), ref["g16"].double()
    box = float((o16[..., :4] - o32[..., :4]).abs().max() / o32[..., :4].abs().max())
    att = float((o16[..., 4] - o32[..., 4]).abs().max() / o32[..., 4].abs().max())
    l32, l16 = float(ref["l32"]["loss"].double().mean()), float(ref["l16"]["loss"].double().mean())
    rel_loss = abs(l16 - l32) / abs(l32)
    l2 = float((g16 - g32).norm() / g32.norm())
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    net = ref["net32"]
    for name in net._param_names:
        a, b = grad_of(net, g32, name), grad_of(net, g16, name)
        if float(a.norm()) > 0:
            print(f"bf16_head parity {name:48s} l2 {float((b - a).norm() / a.norm()):.3e}")
    print(f"bf16_head parity: box {box:.3e} att {att:.3e} loss {rel_loss:.3e} ({l32:.6f} -> {l16:.6f}) flat l2 {l2:.3e} 1-cos {1 - cos:.3e}")
    assert not torch.equal(bits(ref["g16"]), bits(ref["g32"])), "the gradient equals the fp32 plan's bit for bit: the switch is not engaged"
    assert not torch.equal(bits(ref["o16"]), bits(ref["o32"]))
    assert math.isfinite(l16) and bool(torch.isfinite(g16).all())
    assert box <= BOUND_BOX and att <= BOUND_ATT, (box, att)
    assert rel_loss <= BOUND_LOSS, rel_loss
    assert l2 <= BOUND_L2 and cos >= BOUND_COS, (l2, cos)


def test_two_bf16_steps_are_bit_identical(Z, ref):
    o, _, g = step(Z, ref["cfg16"], ref["net16"], ref["inp"])
    assert torch.equal(bits(g), bits(ref["g16"])) and torch.equal(bits(o), bits(ref["o16"]))


def test_fresh_weights_after_an_optimizer_step(Z, ref):
    """the packed images follow the optimizer: after FusedAdam.step() a head layer's forward and data gradient match the UPDATED
    parameters and miss the old ones"""
    cfg, net = build(Z, train_dtype="bf16_head")
    opt = Z["optim"].FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    lf = loss_fn(Z, cfg)
    net.train()
    opt.zero_grad()
    lf(net(ref["inp"]), ref["inp"])["loss"].mean().backward()
    old = net.store.flat.detach().cpu().clone()
    opt.step()
    opt.zero_grad()
    out = net(ref["inp"])
    lf(out, ref["inp"])["loss"].mean().backward()
    torch.cuda.synchronize()
    new = net.store.flat.detach().cpu().clone()
    assert not torch.equal(old, new)
    plan = train_plan(net)
    layer = HEAD + "2.0"
    for kind, what in (("fwd", layer), ("dgrad", "dgrad:" + layer)):
        (e,) = [e for e in plan._b16_log if (e["kind"], e["what"]) == (kind, what)]
        fresh, stale = local_check(net, plan, e, new), local_check(net, plan, e, old)
        print(f"bf16_head fresh weights {kind} {layer}: error / bound {fresh:.4f} against the updated parameters, {stale:.1f} against the old ones")
        assert fresh <= 1.0, (kind, fresh)
        assert stale > 1.0, f"{kind}: the launch also matches the parameters before the optimizer step"


def test_switching_back_gives_fp32_bits_and_eval_ignores_the_switch(Z, ref):
    cfg, net = build(Z)
    assert net.train_precision("bf16_head") is net
    _, _, g16 = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g16), bits(ref["g16"]))
    assert net.train_precision("fp32") is net
    _, _, g32 = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g32), bits(ref["g32"]))
    assert [k for k in net._plans if k[-1]] == [k for k in ref["net32"]._plans if k[-1]], "one training plan, the fp32 key"
    _, n32 = build(Z)
    for _ in range(2):
        step(Z, cfg, n32, ref["inp"])
    # (the two nets' encoders ran the same two training forwards: the same running statistics)
    assert torch.equal(bits(net._rmv), bits(n32._rmv))
    net.train_precision("bf16_head")
    net.eval()
    n32.eval()
    with torch.no_grad():
        a, b = net(ref["inp"])["att_bbx_out"], n32(ref["inp"])["att_bbx_out"]
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b))
    ek = [k for k in net._plans if not k[-1]]
    assert ek == [k for k in n32._plans if not k[-1]] and len(ek) == 1
    assert listing(net._plans[ek[0]].fwd) == listing(n32._plans[ek[0]].fwd) and not net._plans[ek[0]]._b16_log


def test_frozen_encoder(Z, ref):
    cfg, net = build(Z, train_dtype="bf16_head")
    for n, p in net.named_parameters():
        p.requires_grad_(not n.startswith(ENC))
    _, _, g = step(Z, cfg, net, ref["inp"])
    plan, full = train_plan(net), train_plan(ref["net16"])
    assert [w for _, n, w in listing(plan.fwd) if "bf16" in n] == [w for _, n, w in listing(full.fwd) if "bf16" in n]
    assert sorted(w for _, n, w in listing(plan.bwd) if n == "zsg_conv_igemm_bf16_m") == sorted("dgrad:" + n + "+bf16" for n in DGRAD_LAYERS)
    assert not any(w.startswith("dgrad:" + FPN + nm) for _, _, w in listing(plan.bwd) for nm in ("P3_1", "P4_1", "P5_1", "P6")), "nothing trains upstream"
    for name in net._param_names:
        if name.startswith(ENC):
            assert not bool(grad_of(net, g, name).any()), name
        else:
            assert torch.equal(bits(grad_of(net, g, name)), bits(grad_of(net, ref["g16"], name))), name


def test_shared_training_conv0(Z):
    """4 queries over 2 images: conv0's feature GEMM leaves Y per image slot, its data gradient reads the segmented sum dY"""
    inp = shared_batch(Z)
    cfg, net = build(Z, train_dtype="bf16_head")
    net.shared_training(True)
    o, ls, g = step(Z, cfg, net, inp)
    (key,) = [k for k in net._plans if k[-1]]
    assert ("shared", 4) in key and ("train", "bf16_head") in key
    plan = train_plan(net)
    (ef,) = [e for e in plan._b16_log if e["kind"] == "fwd" and e["what"] == HEAD + "0.0.feat"]
    (ed,) = [e for e in plan._b16_log if e["kind"] == "dgrad" and e["what"] == "dgrad:" + HEAD + "0.0"]
    assert ef["out"].name.endswith(".Y") and ef["out"].B == 2 and ed["src"].name.endswith(".dY") and ed["src"].B == 2 and ed["out"].B == 2
    assert ef["window"] == (0, 256) and ed["window"] == (0, 256) and ef["add"] is None and ed["add"] is None and ef["d"].relu == 0
    # every launch of that plan (conv0's replayed data gradient last, see REPLAY)
    res = check_all(net, plan, o, ["dgrad:" + FPN + "P4_2", "dgrad:" + FPN + "P5_2"])
    for e in (ef, ed):
        v = res[(e["kind"], e["what"])]
        print(f"bf16_head shared training {e['kind']} {e['what']}: max |out - ref| / bound = {v:.4f}")
        assert v <= 1.0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(ls["loss"]).all())


def test_two_steps_with_clipping_and_adam_stay_finite(Z, ref):
    cfg, net = build(Z, train_dtype="bf16_head", wgrad_dtype="bf16")
    opt = Z["optim"].FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))
    w0 = net.store.flat.clone()
    lf = loss_fn(Z, cfg)
    net.train()
    for _ in range(2):
        opt.zero_grad()
        ls = lf(net(ref["inp"]), ref["inp"])
        ls["loss"].mean().backward()
        tn = Z["optim"].clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tn)) and float(tn) > 0 and bool(torch.isfinite(net.store.flat).all()) and bool(torch.isfinite(ls["loss"]).all())
    assert not torch.equal(net.store.flat, w0)

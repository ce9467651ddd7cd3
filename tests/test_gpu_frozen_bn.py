"""Frozen (eval-mode) BatchNorm layers inside a training network ("Frozen BatchNorm").
  * C ABI: zsg_bn_frozen_backward / zsg_bn_frozen_relu_maxpool_bwd against torch fp64 autograd of F.batch_norm(training=False)
    (+ ReLU bits, + residual gradient, + max_pool2d for the stem), every nullable output, accumulate, the partials form, and
    bit-identical repeats.
  * Plan, ResNet-18, 96 px, B = 2: outputs, loss and gradients against the oracle with a per-layer BatchNorm mode; frozen layers'
    running statistics and counters bit-identical after three FusedAdam steps; no statistics launch for a frozen layer.
  * Plan, configs[1] shape (ResNet-50, 300^2, B = 16), every layer frozen: outputs and sampled gradients against the oracle-made
    fixture tests/golden/o3_r50_300_b16_frozen_bn.npz (fp64 + the CPU-fp32 yard-stick), the eval plan's outputs against the same,
    deterministic gradients under ZSG_DETERMINISTIC=1, and the backward forms that ran (bnb-fused, aliased residual, stem, bnpre)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

RATIOS, SCALES = O.default_ratios_scales()
ENC = "backbone.encoder."


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, loss, mdl, optim
    return _lib, config, loss, mdl, optim


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(m):
    """packed ReLU bits as zsg_bn_apply writes them: byte j holds elements 4j..4j+3 (bit e = element 4j+e)"""
    m = m.reshape(-1, 4).to(torch.uint8)
    return (m[:, 0] | (m[:, 1] << 1) | (m[:, 2] << 2) | (m[:, 3] << 3)).contiguous()


def _eval_ref(x, dout_g, rm, rv, gamma, beta):
    """fp64 autograd of F.batch_norm(training=False) for grad_output g: (dx, dgamma, dbeta)"""
    x64 = x.double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.batch_norm(x64, rm.double(), rv.double(), g64, b64, False, 0.1, 1e-5)
    y.backward(dout_g.double())
    return x64.grad, g64.grad, b64.grad


KCASES = [  # rows, C, mask, residual gradient, dx, sums, accumulate, partials
    (333, 64, True, True, True, True, False, False),
    (1027, 256, False, False, True, True, True, False),
    (77, 2048, True, False, True, True, False, False),
    (333, 64, True, False, False, True, True, False),       # the input needs no gradient
    (513, 256, True, True, True, False, False, False),      # frozen affine: a pure scale
    (1027, 256, True, False, True, True, True, True),       # sums from a data gradient's partial rows
    (77, 2048, False, True, True, True, False, True),
]


@pytest.mark.parametrize("case", KCASES, ids=[f"k{i}" for i in range(len(KCASES))])
def test_frozen_backward_c_abi(Z, case):
    L = Z[0]
    rows, C, use_mask, use_gout, use_dx, sums, acc, use_part = case
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    dout = torch.randn(rows, C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) * 2 + 0.2
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    m = torch.rand(rows, C, generator=g) > 0.4 if use_mask else torch.ones(rows, C, dtype=torch.bool)
    ge = dout * m
    dx_ref, dg_ref, db_ref = _eval_ref(x, ge, rm, rv, gamma, beta)
    invstd = (1.0 / torch.sqrt(rv + 1e-5)).float()
    prev_g, prev_b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    cu = {k: v.cuda() for k, v in dict(x=x, dout=dout, rm=rm, inv=invstd, gamma=gamma).items()}
    bits = _bits(m.flatten()).cuda() if use_mask else None
    part, chunks = None, 0
    if use_part:                # partial rows over an uneven split, as an epilogue would leave them
        cuts = [0, rows // 7, rows // 3, rows // 2 + 5, rows]
        xh = (x - rm) * invstd
        part = torch.stack([torch.stack([ge[a:b].sum(0), (ge[a:b] * xh[a:b]).sum(0)]) for a, b in zip(cuts[:-1], cuts[1:])]).cuda()
        chunks = len(cuts) - 1
    ws_bytes = int(L.lib.zsg_bn_workspace_bytes(rows, C))
    ws = torch.empty(ws_bytes // 4, device="cuda")

    def run():
        dx = torch.full((rows, C), float("nan"), device="cuda") if use_dx else None
        go = torch.full((rows, C), float("nan"), device="cuda") if use_gout else None
        dg = (prev_g.clone() if acc else torch.full((C,), float("nan"))).cuda() if sums else None
        db = (prev_b.clone() if acc else torch.full((C,), float("nan"))).cuda() if sums else None
        L.check(L.lib.zsg_bn_frozen_backward(cu["dout"].data_ptr(), _p(bits), cu["x"].data_ptr() if sums and not use_part else None, rows, C,
                                             cu["rm"].data_ptr(), cu["inv"].data_ptr(), cu["gamma"].data_ptr(), _p(dx), _p(go), _p(dg), _p(db),
                                             int(acc), _p(part), chunks, ws.data_ptr() if sums else None, ws_bytes if sums else 0,
                                             L.stream_ptr()), "frozen_backward")
        torch.cuda.synchronize()
        return [t.cpu() if t is not None else None for t in (dx, go, dg, db)]
    dx, go, dg, db = run()
    if use_dx:
        assert float((dx.double() - dx_ref).abs().max()) <= 1e-5 * float(dx_ref.abs().max())
    if use_gout:
        assert torch.equal(go, ge)
    if sums:
        dg_ref = dg_ref + (prev_g.double() if acc else 0)
        db_ref = db_ref + (prev_b.double() if acc else 0)
        assert float((dg.double() - dg_ref).abs().max()) <= 1e-5 * rows ** 0.5 * float(dg_ref.abs().max() + 1)
        assert float((db.double() - db_ref).abs().max()) <= 1e-5 * rows ** 0.5 * float(db_ref.abs().max() + 1)
    again = run()
    assert all(a is None or torch.equal(a, b) for a, b in zip(again, (dx, go, dg, db))), "two identical launches differ"


@pytest.mark.parametrize("B,H,W,C,sums,acc", [(2, 19, 23, 64, True, True), (3, 10, 9, 256, True, False), (2, 11, 11, 64, False, False)])
def test_frozen_relu_maxpool_bwd_c_abi(Z, B, H, W, C, sums, acc):
    L = Z[0]
    g = torch.Generator().manual_seed(B * H * W + C)
    x = torch.randn(B, H, W, C, generator=g) * 1.3 + 0.2
    rm, rv = torch.randn(C, generator=g) * 0.4, torch.rand(C, generator=g) * 2 + 0.3
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    dout = torch.randn(B, Ho, Wo, C, generator=g)
    prev_g, prev_b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    invstd = (1.0 / torch.sqrt(rv + 1e-5)).float()
    cx, cm, ci, cg, cb = x.cuda(), rm.cuda(), invstd.cuda(), gamma.cuda(), beta.cuda()
    out = torch.empty(B, Ho, Wo, C, device="cuda")
    idx = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device="cuda")
    L.check(L.lib.zsg_bn_relu_maxpool_fwd(cx.data_ptr(), B, H, W, C, cm.data_ptr(), ci.data_ptr(), cg.data_ptr(), cb.data_ptr(), 3, 2, 1,
                                          Ho, Wo, out.data_ptr(), idx.data_ptr(), L.stream_ptr()), "fwd")
    # fp64 reference: max_pool2d(relu(batch_norm_eval(x)))
    x64 = x.permute(0, 3, 1, 2).double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.max_pool2d(F.relu(F.batch_norm(x64, rm.double(), rv.double(), g64, b64, False, 0.1, 1e-5)), 3, 2, 1)
    assert float((out.cpu().permute(0, 3, 1, 2).double() - y.detach()).abs().max()) < 1e-4
    y.backward(dout.permute(0, 3, 1, 2).double())
    ws_bytes = int(L.lib.zsg_bn_workspace_bytes(B * H * W, C))
    ws = torch.empty(ws_bytes // 4, device="cuda")
    cd = dout.cuda()

    def run():
        dx = torch.full((B, H, W, C), float("nan"), device="cuda")
        dg = (prev_g.clone() if acc else torch.full((C,), float("nan"))).cuda() if sums else None
        db = (prev_b.clone() if acc else torch.full((C,), float("nan"))).cuda() if sums else None
        L.check(L.lib.zsg_bn_frozen_relu_maxpool_bwd(cd.data_ptr(), idx.data_ptr(), cx.data_ptr(), B, H, W, C, cm.data_ptr(), ci.data_ptr(),
                                                     cg.data_ptr(), cb.data_ptr(), 3, 2, 1, Ho, Wo, dx.data_ptr(), _p(dg), _p(db), int(acc),
                                                     ws.data_ptr() if sums else None, ws_bytes if sums else 0, L.stream_ptr()), "bwd")
        torch.cuda.synchronize()
        return [t.cpu() if t is not None else None for t in (dx, dg, db)]
    dx, dg, db = run()
    dx_ref = x64.grad.permute(0, 2, 3, 1)
    assert float((dx.double() - dx_ref).abs().max()) <= 1e-5 * float(dx_ref.abs().max())
    if sums:
        n = (B * H * W) ** 0.5
        dg_ref, db_ref = g64.grad + (prev_g.double() if acc else 0), b64.grad + (prev_b.double() if acc else 0)
        assert float((dg.double() - dg_ref).abs().max()) <= 1e-5 * n * float(dg_ref.abs().max() + 1)
        assert float((db.double() - db_ref).abs().max()) <= 1e-5 * n * float(db_ref.abs().max() + 1)
    again = run()
    assert all(a is None or torch.equal(a, b) for a, b in zip(again, (dx, dg, db))), "two identical launches differ"


# ---- plan level ------------------------------------------------------------------------------------------------------------
class PerLayerBN(O.BNState):
    """the oracle's BatchNorm with torch's per-module mode: layers in `frozen` run F.batch_norm(training=False) in a training forward"""
    frozen = frozenset()

    def __call__(self, x, name):
        if self.training and name in self.frozen:
            sd = self.sd
            return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                                False, 0.1, 1e-5)
        return super().__call__(x, name)


def _stats_sd(arch, seed, B, hw):
    """seeded weights whose running statistics are the batch statistics of another synthetic batch (with the seeded 0 / 1
    statistics a frozen trunk would not normalise)"""
    sd = O.seeded_state_dict(arch, seed)
    rec = {}

    class Rec(O.BNState):
        def __call__(self, x, name):
            rec[name] = (x.mean((0, 2, 3)).detach(), x.var((0, 2, 3)).detach())
            return super().__call__(x, name)
    bt = O.synthetic_batch(B, hw, hw, seed=97)
    g = torch.Generator().manual_seed(3)
    h0, c0 = torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)
    keep = O.BNState
    O.BNState = Rec
    try:
        with torch.no_grad():
            O.zsgnet_forward({k: v.clone() for k, v in sd.items()}, bt, h0, c0, arch=arch)
    finally:
        O.BNState = keep
    for name, (m, v) in rec.items():
        sd[name + ".running_mean"] = m.float().clone()
        sd[name + ".running_var"] = v.float().clone()
    return sd


STATS_FNS = ("zsg_bn_stats", "zsg_bn_stats_from_partials", "zsg_bn_apply_from_partials")


def _conv_of(bn_name):
    if bn_name.endswith("downsample.1"):
        return bn_name[:-1] + "0"
    return bn_name[:-3] + "conv" + bn_name[-1]


def _statistics_launches(plan, frozen):
    """forward launches that compute batch statistics for a frozen layer: the statistics entry points named after it, and the
    *_bnstat / fused-partials convolutions that feed it"""
    bad = []
    convs = {_conv_of(n) for n in frozen}
    for fn, args, what in plan.fwd.calls:
        name = getattr(fn, "__name__", "")
        if name in STATS_FNS and any(what == n or what.endswith(":" + n) for n in frozen):
            bad.append(what)
        if "bnstat" in what and what.split("+")[0] in convs:
            bad.append(what)
        if name in ("zsg_conv_igemm", "zsg_conv_wino") and what in convs:
            pa = args[7]
            if getattr(pa, "value", pa) is not None:
                bad.append(what + " (partials)")
    return bad


def _grad_bad(net, sd, sd64, names):
    bad, ps = [], dict(net.named_parameters())
    for n in names:
        g64 = sd64[n].grad.flatten()
        e = float((ps[n].grad.cpu().double().flatten() - g64).norm())
        ec = float((sd[n].grad.double().flatten() - g64).norm())
        if e > max(6 * ec + 2e-4 * float(g64.norm()), 1.5e-2 * float(g64.norm())) + 1e-9:       # test_gpu_finetune's rule
            bad.append((n, e / (float(g64.norm()) + 1e-30)))
    return bad


FROZEN_SETS = {"all": ("",), "stem": (ENC + "bn1",), "block": (ENC + "layer2.0.",)}


@pytest.mark.parametrize("affine", ["affine", "noaffine"])
@pytest.mark.parametrize("which", list(FROZEN_SETS))
def test_plan_frozen_bn_vs_oracle(Z, which, affine, monkeypatch):
    L, config, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    sd = _stats_sd("resnet18", 11, 2, 96)
    net.load_state_dict(sd)
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    frozen = set(net.freeze_batchnorm(FROZEN_SETS[which]))
    assert frozen and (which != "block" or ENC + "layer2.0.downsample.1" in frozen)
    if affine == "noaffine":            # FrozenBatchNorm2d: eval mode and gamma / beta not trained
        for n, p in net.named_parameters():
            if n.rsplit(".", 1)[0] in frozen:
                p.requires_grad_(False)
    trainable = [n for n, p in net.named_parameters() if p.requires_grad]
    bt = O.synthetic_batch(2, 96, 128, seed=5, tmax=13)
    gq = torch.Generator().manual_seed(2)
    h0, c0 = torch.randn(2, 2, 128, generator=gq), torch.randn(2, 2, 128, generator=gq)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    bufs0 = {k: v.detach().cpu().clone() for k, v in net.named_buffers()}
    out = net(inp)
    ls = lf(out, inp)
    ls["loss"].backward()
    torch.cuda.synchronize()
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    assert plan.frozen_bn == frozen
    bad = _statistics_launches(plan, frozen)
    assert not bad, bad
    assert sum(1 for c in plan.fwd.calls if c[2].startswith("eval stats")) == 1
    # which backward form each frozen layer got (what the oracle comparison below covers)
    paths = plan.frozen_bn_paths
    print(f"{which}/{affine} frozen backward forms:", sorted(set(paths.values())))
    assert set(paths) <= frozen and (affine == "noaffine" or set(paths) == frozen)
    if affine == "affine" and which == "all":
        assert any(v.startswith("bnb") for v in paths.values()), "no bnb-fused frozen backward at the small shape"
    # the oracle with the same per-layer modes
    monkeypatch.setattr(O, "BNState", type("PL", (PerLayerBN,), {"frozen": frozenset(frozen)}))
    for k, v in sd.items():
        if v.is_floating_point() and k in trainable:
            v.requires_grad_()
    ref = O.zsgnet_forward(sd, bt, h0, c0, arch="resnet18")
    fs = [tuple(x) for x in ref["feat_sizes"].tolist()]
    anc = torch.from_numpy(O.create_anchors(fs, RATIOS, SCALES).astype(np.float32))
    lref = O.torch_loss(ref, bt["annot"], anc)
    lref["loss"].backward()
    err = float((out["bbx_out"].detach().cpu() - ref["bbx_out"].detach()).abs().max())
    assert err < 2e-3, err
    assert abs(ls["loss"].item() - lref["loss"].item()) < 2e-4 * abs(lref["loss"].item()) + 1e-6
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ref64 = O.zsgnet_forward(sd64, {k: v.double() for k, v in bt.items()}, h0.double(), c0.double(), arch="resnet18", rank=O.sort_rank(bt["qlens"]))
    O.torch_loss(ref64, bt["annot"], anc)["loss"].backward()
    bad = _grad_bad(net, sd, sd64, trainable)
    assert not bad, bad[:8]
    # three optimizer steps: frozen layers' statistics and counters stay put, bit for bit; train-mode layers' move
    opt = optim.FusedAdam(net, lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        lf(net(inp), inp)["loss"].backward()
        opt.step()
    torch.cuda.synchronize()
    bufs = {k: v.detach().cpu() for k, v in net.named_buffers()}
    for name in net.bns:
        for leaf in ("running_mean", "running_var", "num_batches_tracked"):
            k = name + "." + leaf
            if name in frozen:
                assert torch.equal(bufs[k], bufs0[k]), k
            else:
                assert not torch.equal(bufs[k], bufs0[k]), k
    assert all(int(bufs[n + ".num_batches_tracked"] - bufs0[n + ".num_batches_tracked"]) == 4 for n in net.bns if n not in frozen)


def _o3_net(Z):
    """configs[1] network with the o3 fixture's weights and running statistics (tests/golden/make_frozen_bn_fixture.py)"""
    L, config, loss, mdl, optim = Z
    o3 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "o3_r50_300_b16_frozen_bn.npz"))
    cfg = config.get_cfg(resnet_arch="resnet50")
    net = mdl.get_default_net(9, cfg)
    sd = O.seeded_state_dict("resnet50", int(o3["seed"][0]))
    off = 0
    for n in o3["bn_names"]:
        n = str(n)
        c = net.bns[n].c
        sd[n + ".running_mean"] = torch.from_numpy(o3["running_mean"][off:off + c].copy())
        sd[n + ".running_var"] = torch.from_numpy(o3["running_var"][off:off + c].copy())
        off += c
    assert off == o3["running_mean"].size and len(o3["bn_names"]) == len(net.bns) == 53
    net.load_state_dict(sd)
    net.to("cuda").train()
    bt = O.synthetic_batch(16, 300, 300, seed=int(o3["batch_seed"][0]))
    g = torch.Generator().manual_seed(int(o3["hc_seed"][0]))
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, 16, 128, generator=g), torch.randn(2, 16, 128, generator=g)
    r, s = config.ratios_scales(cfg)
    return o3, net, inp, loss.get_default_loss(r, s, cfg)


def test_configs1_all_frozen_vs_oracle_fixture(Z):
    """every BatchNorm frozen at the configs[1] shape, gamma / beta trainable: the shape that reaches the fused stem, the deferred
    (bnpre) apply and the bnb-fused frozen backward in its in-kernel-finalize and partial-row forms, with the residual gradient aliased.
    Outputs and sampled gradients against the fp64 oracle with the CPU-fp32 oracle's own distance as the yard-stick (test_gpu_fullshape's
    rule); the eval plan (BatchNorm folded into the convolutions) against the same fp64 outputs; two deterministic steps bit-identical."""
    L = Z[0]
    o3, net, inp, lf = _o3_net(Z)
    o64, st = torch.from_numpy(o3["out64_s"]), int(o3["out_stride"][0])
    f_cpu = float(o3["fwd_err_cpu"][0])
    bound = max(4 * f_cpu, 2e-3)
    net.eval()
    with torch.no_grad():
        ev = net(inp)["att_bbx_out"].detach().cpu().double()[:, ::st]
    net.train()
    assert len(net.freeze_batchnorm()) == 53
    old = os.environ.get("ZSG_DETERMINISTIC")
    os.environ["ZSG_DETERMINISTIC"] = "1"
    L.lib.zsg_set_deterministic(1)
    try:
        grads = []
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            out = net(inp)
            ls = lf(out, inp)
            ls["loss"].backward()
            torch.cuda.synchronize()
            grads.append(net.store.grad.clone())
    finally:
        if old is None:
            os.environ.pop("ZSG_DETERMINISTIC", None)
        else:
            os.environ["ZSG_DETERMINISTIC"] = old
        L.lib.zsg_set_deterministic(1 if old == "1" else 0)
    f_hip = float((out["att_bbx_out"].detach().cpu().double()[:, ::st] - o64).abs().max())
    f_ev = float((ev - o64).abs().max())
    print(f"forward max abs err vs fp64: frozen training plan {f_hip:.2e}, eval plan {f_ev:.2e}, CPU fp32 oracle {f_cpu:.2e}")
    assert f_hip <= bound and f_ev <= bound, (f_hip, f_ev, f_cpu)
    np.testing.assert_allclose(ls["loss"].item(), float(o3["loss64"][0]), rtol=2e-4)
    assert torch.equal(grads[0], grads[1]), "two identical deterministic steps differ"
    # sampled gradients against fp64, next to the CPU fp32 oracle's distance (test_gpu_fullshape.py)
    P, rows = dict(net.named_parameters()), []
    for i, n in enumerate(o3["names"]):
        n = str(n)
        gh = P[n].grad.detach().cpu().double().reshape(-1)
        k = gh.numel()
        idx = np.arange(0, k, max(1, k // 128))[:128]
        g64s, g32s = torch.from_numpy(o3["g64_s"][i][:len(idx)]), torch.from_numpy(o3["g32_s"][i][:len(idx)]).double()
        sc = (k / len(idx)) ** 0.5
        n64 = float(o3["norm64"][i]) + 1e-300
        rows.append((float((gh[idx] - g64s).norm()) * sc / n64, max(float(o3["err32"][i]), float((g32s - g64s).norm()) * sc) / n64, n))
    w = max(rows)
    print(f"vs fp64: worst HIP rel err {w[0]:.2e} ({w[2]}; CPU fp32 there {w[1]:.2e})")
    bad = [(n, a, b) for a, b, n in rows if a > max(4 * b, 2e-3)]
    assert not bad, bad[:8]
    assert len(rows) == len([p for p in net.parameters() if p.grad is not None])
    # what this covered
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    assert not _statistics_launches(plan, set(net.bns))
    paths = plan.frozen_bn_paths
    print("frozen backward forms:", sorted(set(paths.values())))
    assert set(paths) == set(net.bns)
    assert any(v.startswith("bnb+fin") for v in paths.values()) and any(v.startswith("bnb") and not v.startswith("bnb+fin") for v in paths.values())
    assert any(v.endswith("+alias") for v in paths.values()) and paths["backbone.encoder.bn1"] == "stem+sums"
    assert any("+bnpre(" in c[2] for c in plan.fwd.calls), "the deferred apply stays, fed the eval statistics"

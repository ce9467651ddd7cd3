"""enc_bwd_dtype = "bf16" on the network: ZSGNet.encoder_backward_precision / cfg enc_bwd_dtype, the training plan whose encoder data
gradients behind the stem run on zsg_conv_igemm_bf16_m and, where one completes a BatchNorm's dout, on zsg_conv_igemm_bf16_bnb (that
BatchNorm's backward partial rows in the epilogue).  The set-up of tests/test_gpu_net_enc_bf16.py: ResNet-18, 128 px, B = 2,
O.seeded_state_dict("resnet18", 1), O.synthetic_batch(2, 128, 128, seed=3), fixed h0 / c0, under ZSG_DETERMINISTIC=1; one ResNet-50 case
for bottlenecks, the residual alias (epi_flags bit 0) and the bnpre consumers.

Exact part: the forward is untouched (outputs, loss, running statistics), and so is every gradient whose dout does not pass through a
covered data gradient: the heads, the pyramid, the language / LSTM parameters, and the encoder's last block's closing convolution and
BatchNorm (their dout comes from the pyramid's fp32 data gradients only).  With the switch back at "fp32" a step gives the fp32 bits.

Layer-local part (the rigorous one): every "enc_dgrad" entry of plan._b16_log is observed in a second, identical step whose logged
launches are wrapped on the host (the buffer a launch accumulates into is copied in front of it, its output, operands and partial rows
behind it; the BatchNorm backward that follows a re-issued launch likewise):
  * the data gradient, recomputed on the host from the GPU's OWN dy bits and the current parameters, both rounded to bf16 (torch's
    round-to-nearest-even), fp64 sums, plus the buffer's earlier content, under the project's bound |out - ref| <= (K + 4) * 2^-23 * S,
    K = taps * C, S the same sum of absolute values (tests/test_gpu_conv_bf16.py); with epi_flags bit 0 the masked elements are zero;
  * the partial rows against fp64 sums over the kernel's own stored rows (masked on the host where the kernel stored v; the rows of a
    tile from the descriptor: a strided data gradient has one segment per stride-parity class):
    |sum g - ref| <= (BM - 1) * 2^-24 * sum |g|, |sum g * xhat - ref| <= (BM + 3) * 2^-24 * sum |g * xhat| (tests/test_gpu_conv_bf16_bnb.py);
  * the BatchNorm's d(beta) / d(gamma) against the fp64 sums P of the GPU's own partial rows: `chunks` rows are added (at most chunks - 1
    fp32 additions, each off by at most 2^-24 of a partial sum <= A = sum |row|) and the result is rounded once: <= chunks * 2^-24 * A;
  * the BatchNorm's dx = gamma * invstd * (g - c1 - xhat * c2), c1 = P1 / n, c2 = P2 / n, xhat = (x - mean) * invstd.  However the
    kernel orders the expression (coefficient forms a * g + b * x + c included, where x and mean no longer cancel first), it makes at most
    12 fp32 roundings (2 for the c's, 2 for xhat or its coefficients, one per product, sum and difference), each relative to a term of
    M = |gamma * invstd| * (|g| + |c1| + (|x| + |mean|) * invstd * |c2|); the c's carry dc = chunks * 2^-24 * A / n:
    |dx - ref| <= 12 * 2^-24 * M + |gamma * invstd| * (dc1 + (|x| + |mean|) * invstd * dc2).

Rounded part against the fp32 plan: the flat gradient's relative L2 and 1 - cosine, bounded by 1.5 x what the CPU emulation gives for
the same set-up (tools/enc_bwd_bf16_emul.py: the oracle with the operands of the encoder's data gradients rounded to bf16; the margin is
for the summation orders).  No number is fixed here; what an MI355X gave is in profiles/enc_bwd_bf16_parity_measured.txt."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

MARGIN = 1.5

ENC = "backbone.encoder."
FPN = "backbone.fpn."
STEM = (ENC + "conv1", ENC + "bn1")
U = 2.0 ** -24


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


def build(Z, arch="resnet18", drop_key=False, **flags):
    cfg = Z["config"].get_cfg(resnet_arch=arch, **flags)
    if drop_key:
        cfg.pop("enc_bwd_dtype")
    net = Z["mdl"].get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict(arch, 1))
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


def enc_dgrads(lst):
    return [(lane, n, w) for lane, n, w in lst if w.startswith("dgrad:" + ENC)]


def is_stem(what):
    return any(what.endswith(s) or (s + "+") in what for s in STEM)


# ---- observing the logged launches of a step --------------------------------------------------------------------------------------------
def observed_step(Z, cfg, net, inp):
    """one more step of `net` (its plan exists) with every "enc_dgrad" launch, and the BatchNorm backward behind a re-issued one, wrapped
    on the host: returns {what: snapshot dict of CPU tensors}.  The program is restored afterwards."""
    plan = train_plan(net)
    calls = plan.bwd.calls
    keep = list(calls)
    snaps = {}

    def cpu(t):
        return t.detach().cpu().clone()
    for e in [e for e in plan._b16_log if e["kind"] == "enc_dgrad"]:
        idx = e["idx"]
        fn, args, what = calls[idx]
        s = snaps[e["what"]] = {}

        def spy(*a, fn=fn, e=e, s=s):
            torch.cuda.synchronize()
            if e["add"] is not None:
                s["add"] = cpu(e["out"].buf)
            rc = fn(*a)
            torch.cuda.synchronize()
            s["out"], s["dy"] = cpu(e["out"].buf), cpu(e["src"].buf)
            if e["mask"] is not None:
                s["mask"] = cpu(e["mask"].buf)
            if e["bn"] is not None:
                n_el = e["chunks"] * 2 * e["d"].N
                s["part"] = cpu(e["part"][:n_el]).view(e["chunks"], 2, e["d"].N)
                s["x"], s["mean"], s["invstd"] = cpu(e["x"].buf), cpu(e["mean"]), cpu(e["invstd"])
                s["rmask"] = cpu(e["rmask"]).view(torch.uint8) if e["rmask"] is not None else None
            return rc
        spy.__name__ = fn.__name__
        calls[idx] = (spy, args, what)
        if e["bn"] is not None:
            fb, ab, wb = calls[idx + 1]
            assert wb.endswith(":" + e["bn"]), (wb, e["bn"])
            s["bn_fn"] = fb.__name__

            def spy_bn(*a, fb=fb, e=e, s=s):
                rc = fb(*a)
                torch.cuda.synchronize()
                if e["x"].grad is not None:
                    s["bn_dx"] = cpu(e["x"].grad.buf)
                ents = net.store.entries
                s["dgamma"] = cpu(net.store.grad[ents[e["bn"] + ".weight"].offset:][:e["d"].N])
                s["dbeta"] = cpu(net.store.grad[ents[e["bn"] + ".bias"].offset:][:e["d"].N])
                return rc
            spy_bn.__name__ = fb.__name__
            calls[idx + 1] = (spy_bn, ab, wb)
    try:
        res = step(Z, cfg, net, inp)
    finally:
        calls[:] = keep
    return snaps, res


def level_view(act, buf, i, Cc):
    lv = act.levels[i]
    return torch.as_strided(buf, (act.B, lv.H, lv.W, Cc), (lv.bstride, lv.W * act.ld, act.ld, 1), lv.off)


def dgrad_ref(dy, w, H, W, k, s, p):
    """dy [B, Ho, Wo, cout], w [cout, k, k, cin] -> dx [B, H, W, cin] (the scatter form of the convolution's transpose)"""
    B, Ho, Wo, co = dy.shape
    buf = torch.zeros(B, H + 2 * p + s, W + 2 * p + s, w.shape[3], dtype=dy.dtype)
    for ty in range(k):
        for tx in range(k):
            buf[:, ty: ty + (Ho - 1) * s + 1: s, tx: tx + (Wo - 1) * s + 1: s] += torch.matmul(dy.reshape(-1, co), w[:, ty, tx]).view(B, Ho, Wo, -1)
    return buf[:, p:p + H, p:p + W].contiguous()


def tile_rows(d, B, H, W, bm):
    """the output rows (indices into the dense [B * H * W] rows of dx) of every M tile of descriptor d at tile height bm, in the kernel's
    order: segment by segment (a strided data gradient has one per stride-parity class), rows (b, y, x) ascending, bm rows per tile"""
    tiles = []
    for i in range(d.nseg):
        sg = d.seg[i]
        b, y, x = torch.meshgrid(torch.arange(B), torch.arange(sg.rows_y), torch.arange(sg.rows_x), indexing="ij")
        idx = (b * H * W + (y * sg.osy + sg.opy) * W + (x * sg.osx + sg.opx)).reshape(-1)
        tiles += [idx[t:t + bm] for t in range(0, idx.numel(), bm)]
    return tiles


def local_check(net, e, s, flat):
    """the observed launch `e` from the GPU's own bits; returns error / bound of (conv, sum g, sum g * xhat, d(beta), d(gamma), BatchNorm dx),
    each <= 1 passes (None: not applicable)"""
    L = net.convs[e["pname"][:-len(".weight")]]
    assert L.dil == 1 and e["kind"] == "enc_dgrad" and len(e["out"].levels) == 1 and len(e["src"].levels) == 1
    ent = net.store.entries[e["pname"]]
    w = flat[ent.offset:ent.offset + L.cout * L.k * L.k * L.cpad].view(L.cout, L.k, L.k, L.cpad)
    d = e["d"]
    row0, n = e["window"]
    assert (d.N, d.C) == (n, e["src"].ld)
    lx = e["out"].levels[0]
    wb = w[..., row0:row0 + n].to(torch.bfloat16).double()
    dy = level_view(e["src"], s["dy"], 0, L.cout).to(torch.bfloat16).double()
    r, S = dgrad_ref(dy, wb, lx.H, lx.W, L.k, L.stride, L.pad), dgrad_ref(dy.abs(), wb.abs(), lx.H, lx.W, L.k, L.stride, L.pad)
    if e["add"] is not None:
        a = level_view(e["out"], s["add"], 0, n).double()
        r, S = r + a, S + a.abs()
    got32 = level_view(e["out"], s["out"], 0, n)
    got = got32.double()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    if e["mask"] is not None:
        on = level_view(e["mask"], s["mask"], 0, n) > 0
        assert bool((got[~on] == 0).all())
        r = torch.where(on, r, torch.zeros_like(r))
    res = [None] * 6
    rows = e["out"].B * lx.H * lx.W
    on = None
    if e["bn"] is not None:
        assert e["out"].ld == n and lx.off == 0 and e["epi_flags"] in (0, 1)
        if s["rmask"] is not None:
            b = s["rmask"][:rows * n // 4].to(torch.int32).view(-1, 1)
            on = ((b >> torch.arange(4, dtype=torch.int32).view(1, 4)) & 1).bool().view(got.shape)
        if e["epi_flags"]:
            assert on is not None and bool((got[~on] == 0).all()), e["what"] + ": a masked element of the stored gradient is not zero"
            r = torch.where(on, r, torch.zeros_like(r))
    else:
        assert "epi_flags" not in e or not e["epi_flags"]
    bound = (L.k * L.k * e["src"].ld + 4) * 2.0 ** -23 * S
    res[0] = float(((got - r).abs() / bound.clamp(min=1e-300)).max())
    if e["bn"] is None:
        return res
    # ---- the partial rows, from the kernel's own stored rows ----
    g = (torch.where(on, got, torch.zeros_like(got)) if on is not None else got).reshape(rows, n)
    x, mean, inv = s["x"][:rows * n].double().view(rows, n), s["mean"].double(), s["invstd"].double()
    xh = (x - mean) * inv
    chunks, part = e["chunks"], s["part"].double()
    bms = [bm for bm in (64, 128) if len(tile_rows(d, e["out"].B, lx.H, lx.W, bm)) == chunks]
    assert bms, (rows, chunks)
    bm = bms[0]                          # (where both tile heights give the same count, no segment exceeds 64 rows: the same tiles)
    tiles = tile_rows(d, e["out"].B, lx.H, lx.W, bm)
    assert sorted(torch.cat(tiles).tolist()) == list(range(rows))
    for which, (term, k_) in enumerate(((g, bm - 1), (g * xh, bm + 3))):
        worst = 0.0
        for t in range(chunks):
            sl = term[tiles[t]]
            err = (part[t, which] - sl.sum(0)).abs()
            worst = max(worst, float((err / (k_ * U * sl.abs().sum(0)).clamp(min=1e-300)).max()))
        res[1 + which] = worst
    if s["bn_fn"] != "zsg_bn_backward_from_partials":
        return res
    # ---- the live BatchNorm's backward, from the GPU's own partial rows ----
    P, A = part.sum(0), part.abs().sum(0)                                # [2, n]
    dsum = chunks * U * A
    res[3] = float(((s["dbeta"].double() - P[0]).abs() / dsum[0].clamp(min=1e-300)).max())
    res[4] = float(((s["dgamma"].double() - P[1]).abs() / dsum[1].clamp(min=1e-300)).max())
    ge = net.store.entries[e["bn"] + ".weight"]
    gi = flat[ge.offset:ge.offset + n].double() * inv
    c1, c2 = P[0] / rows, P[1] / rows
    ref = gi * (g - c1 - xh * c2)
    xm = (x.abs() + mean.abs()) * inv
    M = gi.abs() * (g.abs() + c1.abs() + xm * c2.abs())
    bnd = 12 * U * M + gi.abs() * (dsum[0] / rows + xm * dsum[1] / rows)
    dx = s["bn_dx"][:rows * n].double().view(rows, n)
    res[5] = float(((dx - ref).abs() / bnd.clamp(min=1e-300)).max())
    return res


def check_all(Z, cfg, net, inp, label):
    plan = train_plan(net)
    snaps, res = observed_step(Z, cfg, net, inp)
    flat = net.store.flat.detach().cpu()
    entries = [e for e in plan._b16_log if e["kind"] == "enc_dgrad"]
    assert entries and set(snaps) == {e["what"] for e in entries}
    bad = {}
    for e in entries:
        r = local_check(net, e, snaps[e["what"]], flat)
        fmt = lambda v: "   -  " if v is None else f"{v:.4f}"
        print(f"{label} layer-local {e['what']:52s} error / bound: conv {fmt(r[0])} sum g {fmt(r[1])} sum g*xhat {fmt(r[2])} "
              f"dbeta {fmt(r[3])} dgamma {fmt(r[4])} bn dx {fmt(r[5])}  epi {e.get('epi_flags', '-')}")
        if not all(v is None or v <= 1.0 for v in r):
            bad[e["what"]] = r
    assert not bad, bad
    return entries, res


@pytest.fixture(scope="module")
def ref(Z, deterministic):
    """one step of the fp32 net and of the enc_bwd_dtype = bf16 net on the module's set-up (computed once, never modified)"""
    inp = batch()
    cfg, net32 = build(Z)
    o32, l32, g32 = step(Z, cfg, net32, inp)
    cfg16, net16 = build(Z, enc_bwd_dtype="bf16")
    assert net16._enc_bwd_dtype == "bf16" and net16._enc_dtype == "fp32"
    o16, l16, g16 = step(Z, cfg16, net16, inp)
    return dict(inp=inp, cfg=cfg, cfg16=cfg16, net32=net32, net16=net16, o32=o32, l32=l32, g32=g32, o16=o16, l16=l16, g16=g16)


def check_programs(p32, p16, n_dgrads):
    f32, f16, b32, b16 = listing(p32.fwd), listing(p16.fwd), listing(p32.bwd), listing(p16.bwd)
    assert not any("bf16" in n or "+bf16" in w for prog in (f32, b32, listing(p32.prep), listing(p32.prep_u)) for _, n, w in prog)
    assert not p32._b16_log
    assert f16 == f32 and listing(p16.prep_u) == listing(p32.prep_u), "the forward is the fp32 plan's"
    d32, d16 = enc_dgrads(b32), enc_dgrads(b16)
    assert len(d16) == len(d32) == n_dgrads
    for (l32_, _, w32), (l16_, n16, w16) in zip(d32, d16):
        base = w32.split("+")[0]
        assert l16_ == l32_ and w16 in (base + "+bf16", base + "+bf16+bnb"), (w32, w16)
        assert n16 == ("zsg_conv_igemm_bf16_bnb" if w16.endswith("+bnb") else "zsg_conv_igemm_bf16_m"), (n16, w16)
    assert not any("+bnb+fin" in w for _, _, w in d16), "the bf16 entry has no in-kernel finalize"
    assert any(w.endswith("+bnb") for _, _, w in d16)
    # the stem's and the pyramid's launches are the fp32 plan's
    for pick in (lambda w: is_stem(w), lambda w: FPN in w):
        a, b = [x for x in b32 if pick(x[2])], [x for x in b16 if pick(x[2])]
        assert a and a == b
    # everything that is neither a covered data gradient nor the BatchNorm backward behind one is the fp32 plan's too
    rest = lambda lst: [x for x in lst if not x[2].startswith(("dgrad:" + ENC, "bnbwd:" + ENC, "bnbwd(frozen):" + ENC))]
    assert rest(b16) == rest(b32)
    # ONE more pack launch in the backward's preparation, behind the transpose
    pr32, pr16 = listing(p32.prep), listing(p16.prep)
    assert [n for _, n, _ in pr16].count("zsg_pack_w_bf16_batched") == 1 and not any(n == "zsg_pack_w_bf16_batched" for _, n, _ in pr32)
    assert len(p16.dpack_jobs) == n_dgrads
    log = [e for e in p16._b16_log if e["kind"] == "enc_dgrad"]
    assert len(log) == len(p16._b16_log) == n_dgrads
    for e in log:
        fn, _, what = p16.bwd.calls[e["idx"]]
        assert what.startswith(e["what"] + "+bf16") and (fn.__name__ == "zsg_conv_igemm_bf16_bnb") == (e["bn"] is not None)
        if e["bn"] is not None:
            assert e["chunks"] > 0 and e["mean"].numel() == e["invstd"].numel() == e["d"].N and e["epi_flags"] == e["d"].epi_flags
    return log


def test_programs(Z, ref):
    p32, p16 = train_plan(ref["net32"]), train_plan(ref["net16"])
    (key,) = [k for k in ref["net16"]._plans if k[-1]]
    assert key[-2] == ("encb", "bf16") and not any(isinstance(e, tuple) and e and e[0] == "encb" for e in list(ref["net32"]._plans)[0])
    check_programs(p32, p16, 19)                 # ResNet-18: 16 block convolutions + 3 projections (the stem has no data gradient)


def test_switch_off_lowers_what_a_net_that_never_saw_the_key_lowers(Z, ref):
    cfg, net0 = build(Z, drop_key=True)
    assert "enc_bwd_dtype" not in cfg and net0._enc_bwd_dtype == "fp32"
    o0, _, g0 = step(Z, cfg, net0, ref["inp"])
    p0, p32 = train_plan(net0), train_plan(ref["net32"])
    assert listing(p0.bwd) == listing(p32.bwd) and listing(p0.fwd) == listing(p32.fwd)
    assert listing(p0.prep) == listing(p32.prep) and listing(p0.prep_u) == listing(p32.prep_u)
    assert list(net0._plans) == list(ref["net32"]._plans)
    assert torch.equal(bits(g0), bits(ref["g32"])) and torch.equal(bits(o0), bits(ref["o32"]))


def exact_part(n32, n16, o32, o16, l32, l16, g32, g16):
    assert torch.equal(bits(o16), bits(o32)), "the outputs"
    assert torch.equal(bits(l16["loss"]), bits(l32["loss"])), "the loss"
    assert torch.equal(bits(n16._rm), bits(n32._rm)) and torch.equal(bits(n16._rv), bits(n32._rv)), "the running statistics"
    last = max(int(k.split(".")[3]) for k in n16.store.entries if k.startswith(ENC + "layer4."))
    names = [k for k in n16.store.entries if k.startswith(f"{ENC}layer4.{last}.")]
    tail = max(int(k.split(".")[4][4:]) for k in names if k.split(".")[4].startswith("conv"))
    closing = {f"{ENC}layer4.{last}.conv{tail}.weight", f"{ENC}layer4.{last}.bn{tail}.weight", f"{ENC}layer4.{last}.bn{tail}.bias"}
    assert closing <= set(names)
    checked = 0
    for name in n16.store.entries:
        if name.startswith(ENC) and name not in closing:
            continue
        a, b = grad_of(n16, g16, name), grad_of(n32, g32, name)
        assert torch.equal(bits(a), bits(b)), name
        checked += 1
    assert checked > 20
    rounded = [k for k in n16.store.entries if k.startswith(ENC + "layer1.") and not torch.equal(bits(grad_of(n16, g16, k)), bits(grad_of(n32, g32, k)))]
    assert rounded, "no encoder gradient differs from the fp32 plan's: the switch is not engaged"


def test_exact_part(Z, ref):
    exact_part(ref["net32"], ref["net16"], ref["o32"], ref["o16"], ref["l32"], ref["l16"], ref["g32"], ref["g16"])


def test_layer_local(Z, ref):
    """every covered launch of a step of the net in `ref`, and the BatchNorm backward behind each re-issued one"""
    entries, (o, _, g) = check_all(Z, ref["cfg16"], ref["net16"], ref["inp"], "encb")
    assert len(entries) == 19 and sum(e["bn"] is not None for e in entries) >= 8
    assert torch.equal(bits(g), bits(ref["g16"])) and torch.equal(bits(o), bits(ref["o16"])), "the observed step is the step"


def test_switching_back_gives_fp32_bits_and_two_bf16_steps_are_bit_identical(Z, ref):
    cfg, net = build(Z)
    assert net.encoder_backward_precision("bf16") is net
    o16, _, g16 = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g16), bits(ref["g16"])) and torch.equal(bits(o16), bits(ref["o16"]))
    _, _, g16b = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g16b), bits(ref["g16"])), "two bf16 steps of one net"
    assert net.encoder_backward_precision("fp32") is net
    o32, _, g32 = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g32), bits(ref["g32"])) and torch.equal(bits(o32), bits(ref["o32"]))
    assert [k for k in net._plans if k[-1]] == [k for k in ref["net32"]._plans if k[-1]], "one training plan, the fp32 key"
    # eval ignores the switch
    (_, na), (_, nb) = build(Z, enc_bwd_dtype="bf16"), build(Z)
    na.eval()
    nb.eval()
    with torch.no_grad():
        a, b = na(ref["inp"])["att_bbx_out"], nb(ref["inp"])["att_bbx_out"]
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b)) and list(na._plans) == list(nb._plans)


def test_bottleneck_the_residual_alias_and_the_deferred_batchnorm(Z, monkeypatch):
    """ResNet-50 with the deferral threshold at 0 (a block's closing BatchNorm is applied by the next block's conv1, bnpre): bottleneck
    data gradients, the residual gradient aliased to dout (epi_flags bit 0: the bf16 launch stores the masked gradient)"""
    monkeypatch.setattr(Z["mdl"], "BN_PRE_MIN_MB", 0)
    inp = batch()
    cfg, n32 = build(Z, arch="resnet50")
    o32, l32, g32 = step(Z, cfg, n32, inp)
    cfg16, n16 = build(Z, arch="resnet50", enc_bwd_dtype="bf16")
    o16, l16, g16 = step(Z, cfg16, n16, inp)
    p32, p16 = train_plan(n32), train_plan(n16)
    assert sum("+bnpre(" in w for _, _, w in listing(p16.fwd)) >= 8
    log = check_programs(p32, p16, 52)           # ResNet-50: 48 block convolutions + 4 projections
    assert any(e["bn"] is not None and e["epi_flags"] == 1 for e in log), "no re-issued launch stores the masked gradient"
    assert any(e["bn"] is not None and e["epi_flags"] == 0 for e in log)
    exact_part(n32, n16, o32, o16, l32, l16, g32, g16)
    entries, (_, _, g) = check_all(Z, cfg16, n16, inp, "encb r50")
    assert torch.equal(bits(g), bits(g16))
    assert bool(torch.isfinite(g16).all()) and float(g16.abs().max()) > 0


def test_frozen_encoder_batchnorm(Z, ref):
    """a frozen BatchNorm with trainable gamma / beta: the bf16 launch carries its sums for the eval statistics ("bnb", never "bnb+fin")"""
    cfg, net = build(Z, enc_bwd_dtype="bf16")
    frozen = set(net.freeze_batchnorm((ENC + "layer3.", ENC + "layer4.0.bn1")))
    assert len(frozen) == 6
    _, ls, g = step(Z, cfg, net, ref["inp"])
    plan = train_plan(net)
    entries, _ = check_all(Z, cfg, net, ref["inp"], "encb frozen")
    covered = {e["bn"] for e in entries if e["bn"] is not None}
    assert covered & frozen
    for bn in covered & frozen:
        assert plan.frozen_bn_paths[bn].split("+alias")[0] == "bnb", (bn, plan.frozen_bn_paths[bn])
    assert not any(p.startswith("bnb+fin") for b, p in plan.frozen_bn_paths.items() if b in covered)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(ls["loss"]).all())


def test_shared_training(Z):
    inp = shared_batch(Z)
    cfg, net = build(Z, enc_bwd_dtype="bf16")
    net.shared_training(True)
    _, ls, g = step(Z, cfg, net, inp)
    (key,) = [k for k in net._plans if k[-1]]
    assert ("shared", 4) in key and key[-2] == ("encb", "bf16")
    entries, _ = check_all(Z, cfg, net, inp, "encb shared")
    assert len(entries) == 19 and all(e["out"].B == 2 for e in entries)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(ls["loss"]).all())


def test_all_four_training_switches_together(Z, ref):
    cfg, net = build(Z, enc_bwd_dtype="bf16", enc_dtype="bf16_fwd", train_dtype="bf16_head", wgrad_dtype="bf16")
    cfg3, net3 = build(Z, enc_dtype="bf16_fwd", train_dtype="bf16_head", wgrad_dtype="bf16")
    o, ls, g = step(Z, cfg, net, ref["inp"])
    o3, ls3, g3 = step(Z, cfg3, net3, ref["inp"])
    (key,) = [k for k in net._plans if k[-1]]
    assert key[7:-1] == (("wgrad", "bf16"), ("train", "bf16_head"), ("enc", "bf16_fwd"), ("encb", "bf16"))
    plan, plan3 = train_plan(net), train_plan(net3)
    assert listing(plan.fwd) == listing(plan3.fwd), "the forward is what the other three switches make it"
    assert torch.equal(bits(o), bits(o3)) and torch.equal(bits(ls["loss"]), bits(ls3["loss"]))
    assert sorted({e["kind"] for e in plan._b16_log}) == ["dgrad", "enc_dgrad", "enc_fwd", "fwd"]
    assert [(e["kind"], e["what"]) for e in plan._b16_log if e["kind"] != "enc_dgrad"] == [(e["kind"], e["what"]) for e in plan3._b16_log]
    assert [n for _, n, _ in listing(plan.prep)].count("zsg_pack_w_bf16_batched") == 1, "still one pack launch in the backward's preparation"
    assert len(plan.dpack_jobs) == len(plan3.dpack_jobs) + 19
    for name in net.store.entries:
        if not name.startswith(ENC):
            assert torch.equal(bits(grad_of(net, g, name)), bits(grad_of(net3, g3, name))), name
    check_all(Z, cfg, net, ref["inp"], "encb + enc + head + wgrad")
    assert bool(torch.isfinite(g).all())


def test_two_steps_with_clipping_and_adam_stay_finite(Z, ref):
    cfg, net = build(Z, enc_bwd_dtype="bf16")
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


def test_rounded_part_against_the_fp32_plan(Z, ref):
    from tools import enc_bwd_bf16_emul as emul
    emu_l2, emu_omc = emul.emulate("resnet18", torch.float64)
    g32, g16 = ref["g32"].double(), ref["g16"].double()
    l2 = float((g16 - g32).norm() / g32.norm())
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print(f"enc_bwd_bf16 parity: flat l2 {l2:.3e} 1-cos {1 - cos:.3e}; CPU emulation: flat l2 {emu_l2:.3e} 1-cos {emu_omc:.3e}; "
          f"measured / emulated {l2 / emu_l2:.3f}, {(1 - cos) / emu_omc:.3f} (bound {MARGIN})")
    assert not torch.equal(bits(ref["g16"]), bits(ref["g32"])), "the gradient equals the fp32 plan's bit for bit: the switch is not engaged"
    assert math.isfinite(l2) and bool(torch.isfinite(g16).all()) and emu_l2 > 0 and emu_omc > 0
    assert l2 <= MARGIN * emu_l2, (l2, emu_l2)
    assert 1 - cos <= MARGIN * emu_omc, (1 - cos, emu_omc)

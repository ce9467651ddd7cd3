"""Eval-only shared-image forward (ZSGNet.forward with `img_idx`: Q queries over Bi <= Q images, the image trunk and head conv0's
feature GEMM once per image) against the CPU oracle on the expanded batch img[img_idx], and against today's one-image-per-query path.

Bounds, none of them taken from what the code gives:
  * vs oracle.zsgnet_forward(training=False): the scale-relative bound of test_gpu_net.py::test_eval_mode_and_state_dict_roundtrip
    (2e-4 x the reference's max magnitude, att and bbx), with running statistics set up as there;
  * vs today's GPU path: distance(shared, oracle) <= max(4 x distance(plain, oracle), 2e-3) — the margin test_gpu_fullshape.py allows two
    fp32 routes to one answer;
  * independence of a query's rows from the other queries, from its image's slot and from unused slots: the first bound again."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

CASES = {
    "r18": dict(arch="resnet18", flags={}, hw=128),
    "r50": dict(arch="resnet50", flags={}, hw=128),
    "ssd_vgg": dict(arch="ssd_vgg", flags=dict(mdl_to_use="ssd_vgg"), hw=300),
    "do_norm": dict(arch="resnet50", flags=dict(do_norm=True), hw=128),
    "two_heads": dict(arch="resnet50", flags=dict(use_same_atb=False), hw=128),
}
Q, BI = 8, 3


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import config, mdl, synth
    return config, mdl, synth


def build(Z, tag, seed=3):
    config, mdl, synth = Z
    c = CASES[tag]
    if c["arch"] == "ssd_vgg":
        cfg = config.get_cfg(**c["flags"])
        sd = O.seeded_ssd_state_dict(seed)
    else:
        cfg = config.get_cfg(resnet_arch=c["arch"], **c["flags"])
        sd = O.seeded_state_dict(c["arch"], seed, same_atb=bool(cfg["use_same_atb"]))
    g = torch.Generator().manual_seed(11)
    for k in sd:                                   # non-trivial running statistics (as test_gpu_net.py sets them up)
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
        if k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(sd)
    net.to("cuda").eval()
    return cfg, net, sd


def shared_batch(Z, hw, Bi=BI, q=Q, seed=21):
    _, _, synth = Z
    bt = synth.synthetic_shared_batch(Bi, q, hw, hw, seed=seed)
    gq = torch.Generator().manual_seed(seed + 1)
    bt["h0"], bt["c0"] = torch.randn(2, q, 128, generator=gq), torch.randn(2, q, 128, generator=gq)
    return bt


def to_dev(bt):
    return {k: (v if k in ("h0", "c0") else v.cuda()) for k, v in bt.items()}


def run(net, bt):
    with torch.no_grad():
        out = net(to_dev(bt))
    torch.cuda.synchronize()
    return out["att_out"].cpu(), out["bbx_out"].cpu()


def dist(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("tag", sorted(CASES))
def test_shared_forward_vs_oracle_and_plain_path(Z, tag):
    _, _, synth = Z
    cfg, net, sd = build(Z, tag)
    c = CASES[tag]
    bt = shared_batch(Z, c["hw"])
    assert sorted(set(bt["img_idx"].tolist())) == list(range(BI)) and bt["img_idx"].tolist() != sorted(bt["img_idx"].tolist())
    ex = synth.expand_shared(bt)
    ref = O.zsgnet_forward({k: v.clone() for k, v in sd.items()}, ex, bt["h0"], bt["c0"], arch=c["arch"], training=False,
                           do_norm=bool(cfg["do_norm"]))
    att_s, bbx_s = run(net, bt)
    att_p, bbx_p = run(net, ex)
    assert att_s.shape == ref["att_out"].shape and bbx_s.shape == ref["bbx_out"].shape
    sa, sb = float(ref["att_out"].abs().max()), float(ref["bbx_out"].abs().max())
    ds = (dist(att_s, ref["att_out"]), dist(bbx_s, ref["bbx_out"]))
    dp = (dist(att_p, ref["att_out"]), dist(bbx_p, ref["bbx_out"]))
    print(f"shared-eval parity {tag} (Bi={BI}, Q={Q}, {c['hw']}^2): max|att - oracle| shared {ds[0]:.3e} plain {dp[0]:.3e} (scale {sa:.3e}); "
          f"max|bbx - oracle| shared {ds[1]:.3e} plain {dp[1]:.3e} (scale {sb:.3e}); shared vs plain att {dist(att_s, att_p):.3e} bbx {dist(bbx_s, bbx_p):.3e}")
    assert ds[0] < 2e-4 * sa and ds[1] < 2e-4 * sb
    assert ds[0] <= max(4 * dp[0], 2e-3) and ds[1] <= max(4 * dp[1], 2e-3)


@pytest.mark.parametrize("tag", ["r18", "ssd_vgg"])
def test_query_rows_do_not_depend_on_other_queries_slots_or_padding(Z, tag):
    cfg, net, sd = build(Z, tag)
    hw = CASES[tag]["hw"]
    bt = shared_batch(Z, hw)
    att0, bbx0 = run(net, bt)
    ta, tb = 2e-4 * float(att0.abs().max()), 2e-4 * float(bbx0.abs().max())
    q = 2
    im = int(bt["img_idx"][q])
    # (a) every other query's words replaced.  Their LENGTHS and the drawn initial states stay: the reference's apply_lstm
    # (mdl.py:296-336) sorts the batch by length and hands row r of (h0, c0) to the r-th longest query, so which initial state a
    # query gets depends on the other queries' lengths — in the oracle as here; that is the reference's behaviour, not a leak
    other = shared_batch(Z, hw, seed=77)
    b2 = {k: v.clone() for k, v in bt.items()}
    b2["qvec"] = other["qvec"].clone()
    b2["qvec"][q] = bt["qvec"][q]
    att, bbx = run(net, b2)
    assert dist(att[q], att0[q]) <= ta and dist(bbx[q], bbx0[q]) <= tb, "other queries leak into a query's rows"
    # (b) its image moves to another slot (the images permuted, the index following)
    perm = torch.tensor([1, 2, 0])                  # new slot s holds old image perm[s]
    inv = torch.argsort(perm)
    b3 = {k: v.clone() for k, v in bt.items()}
    b3["img"] = bt["img"][perm]
    b3["img_idx"] = inv[bt["img_idx"]]
    assert int(b3["img_idx"][q]) != im
    att, bbx = run(net, b3)
    assert dist(att, att0) <= ta and dist(bbx, bbx0) <= tb, "the image's slot changes the result"
    # (c) image slots no query points to hold NaN: one inside the batch (Bi = 4 -> no bucket padding), then the padding of the
    # image bucket itself (Bi = 3 in a 4-slot plan whose 4th slot was just filled with NaN by the forward before)
    b4 = {k: v.clone() for k, v in bt.items()}
    b4["img"] = torch.cat([bt["img"], torch.full_like(bt["img"][:1], float("nan"))])
    att, bbx = run(net, b4)
    assert torch.isfinite(att).all() and torch.isfinite(bbx).all(), "an unused image slot reached an output row"
    assert dist(att, att0) <= ta and dist(bbx, bbx0) <= tb
    att, bbx = run(net, bt)
    assert torch.isfinite(att).all() and torch.isfinite(bbx).all(), "the padding of the image bucket reached an output row"
    assert dist(att, att0) <= ta and dist(bbx, bbx0) <= tb


def test_identity_index_agrees_with_plain_forward_and_plain_path_is_untouched(Z, monkeypatch):
    """(in deterministic mode, as test_gpu_bnb.py compares two runs: with fp32-atomic split-K two replays of ONE plan already differ
    in the last bits, and `exactly what it returned before` could not be told from that)"""
    from zsgnet_pytorch_amd import ops
    from zsgnet_pytorch_amd._lib import lib
    saved = dict(ops._TUNE_CACHE)
    monkeypatch.setenv("ZSG_DETERMINISTIC", "1")
    lib.zsg_set_deterministic(1)
    try:
        _identity_and_untouched(Z)
    finally:
        lib.zsg_set_deterministic(0)
        ops._TUNE_CACHE.clear()
        ops._TUNE_CACHE.update(saved)


def _identity_and_untouched(Z):
    _, _, synth = Z
    cfg, net, sd = build(Z, "r18")
    bt = shared_batch(Z, 128, Bi=4, q=4)
    plain = {k: v for k, v in bt.items() if k != "img_idx"}
    att_p, bbx_p = run(net, plain)
    bt["img_idx"] = torch.arange(4)
    att_s, bbx_s = run(net, bt)
    assert dist(att_s, att_p) <= 2e-4 * float(att_p.abs().max()) and dist(bbx_s, bbx_p) <= 2e-4 * float(bbx_p.abs().max())
    att_p2, bbx_p2 = run(net, plain)               # a batch without img_idx after a shared one: exactly what it was
    assert torch.equal(att_p2, att_p) and torch.equal(bbx_p2, bbx_p)
    # int32 indices, uint8 NHWC images
    bt["img_idx"] = torch.arange(4, dtype=torch.int32)
    a2, b2 = run(net, bt)
    assert torch.equal(a2, att_s) and torch.equal(b2, bbx_s)


def test_shared_is_eval_only(Z):
    cfg, net, sd = build(Z, "r18")
    bt = shared_batch(Z, 96, Bi=2, q=3)
    net.train()
    with pytest.raises(RuntimeError, match="eval-only"):
        net(to_dev(bt))
    net.eval()
    out = net(to_dev(bt))                           # grad mode on: the forward runs, a backward through it is refused
    if out["att_bbx_out"].requires_grad:
        with pytest.raises(RuntimeError, match="eval-only"):
            out["att_bbx_out"].sum().backward()
    bad = to_dev(bt)
    bad["img_idx"] = bad["img_idx"][:2]
    with pytest.raises(ValueError):
        net(bad)


@pytest.mark.parametrize("flags", [dict(use_lang=False), dict(use_img=False)], ids=["lang_blind", "img_blind"])
def test_blind_variants_gather_into_the_plain_plan(Z, flags):
    config, mdl, synth = Z
    cfg = config.get_cfg(resnet_arch="resnet50", **flags)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet50", 5, head_in=net.start_dim_head))
    net.to("cuda").eval()
    bt = shared_batch(Z, 96, Bi=2, q=4)
    att_s, bbx_s = run(net, bt)
    att_p, bbx_p = run(net, synth.expand_shared(bt))
    # (the same plan on the same pixels; two replays of one plan differ in the last bits where a split-K launch adds with fp32 atomics)
    assert att_s.shape[0] == 4
    assert dist(att_s, att_p) <= 2e-4 * float(att_p.abs().max()) and dist(bbx_s, bbx_p) <= 2e-4 * float(bbx_p.abs().max())


def test_plan_cache_is_bounded_by_the_image_buckets(Z):
    config, mdl, synth = Z
    cfg, net, sd = build(Z, "r18")
    q = 6
    for Bi in list(range(1, q + 1)) + [3, 1]:
        bt = shared_batch(Z, 64, Bi=Bi, q=q, seed=Bi)
        att, _ = run(net, bt)
        assert att.shape[0] == q and torch.isfinite(att).all()
    shared = [k for k in net._plans if len(k) == 7 and k[5] == "shared"]
    assert len(shared) <= math.ceil(math.log2(q)) + 1, shared
    assert sorted(k[0] for k in shared) == sorted({mdl.bucket_images(b, q) for b in range(1, q + 1)})
    # the cache of shared plans is bounded whatever the stream of geometries
    for qq in range(1, mdl.SHARED_PLANS_MAX + 4):
        run(net, shared_batch(Z, 64, Bi=1, q=qq, seed=qq))
    assert len([k for k in net._plans if len(k) == 7 and k[5] == "shared"]) <= mdl.SHARED_PLANS_MAX

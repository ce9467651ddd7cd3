"""GPU parity of the IoU-aware classification targets fused into the loss kernels (zsg_loss_fwd_bwd_q, cfg cls_quality = "qfl" / "vfl")
through ZSGLoss, against the fp64 restatement of tests/quality_ref.py composed with the oracle's criterion (mask, box_ls, box gradient)
and tests/boxiou_ref.py (the optional IoU loss).  Shapes, seeded inputs and tolerances are those of tests/test_gpu_boxiou.py: loss scalars
(pos_iou included) rel 1e-5; gradients normwise, max|gpu - ref| <= 2e-5 max|ref| per tensor (qfl's derivative is built from s - q, which
cancels where the score meets its target).  Run with -rP to see the measured distances (profiles/quality_parity_measured.txt)."""
import functools

import numpy as np
import pytest
import torch

import quality_ref as Q
from test_gpu_boxiou import GRAD_TOL, LOSS_RTOL, SHAPES, inputs

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

RATIOS, SCALES = O.default_ratios_scales()
GAMMA_ALPHA = [(g, a) for g in (2.0, 1.5) for a in (0.25, 0.75)]
SCALARS = ("loss", "cls_ls", "box_ls", "iou_ls", "pos_iou")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import anchors, config, loss
    return anchors, config, loss


@functools.lru_cache(maxsize=None)
def reference(A, B, disjoint, kind, box_iou, use_multi, gamma, alpha):
    att, reg, annot, anc = inputs(A, B, disjoint)
    return Q.compose(O, att, reg, annot, anc, kind, box_iou, use_multi, alpha, gamma)


def run(M, att, reg, annot, anc, **cfg_kw):
    """ZSGLoss on the GPU -> (losses dict of floats, grad [B,A,5] numpy, match_idx, npos)"""
    anchors, config, loss = M
    gamma = cfg_kw.pop("gamma", None)
    cfg = config.get_cfg(**cfg_kw)
    if gamma is not None:                                # (the override rule keeps a key's type and gamma's default is the int 2)
        cfg["gamma"] = gamma
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    lf.anchs = torch.from_numpy(anc).cuda()
    out5 = torch.cat([torch.from_numpy(reg), torch.from_numpy(att)[..., None]], dim=2).cuda().requires_grad_()
    ls = lf(dict(att_bbx_out=out5, feat_sizes=None, num_f_out=torch.tensor([1])), dict(annot=torch.from_numpy(annot).cuda()))
    assert list(ls) == lf.loss_keys
    assert not ls[lf.loss_keys[-1]].requires_grad
    ls["loss"].backward()
    return ({k: float(v) for k, v in ls.items()}, out5.grad.cpu().numpy(), lf.match_idx.cpu().numpy(), lf.npos.cpu().numpy())


def check(tag, got, grad, ref):
    got = dict(got)
    got.setdefault("iou_ls", 0.0)
    for k in SCALARS:
        print(f"{tag} {k}: gpu {got[k]:.8g} ref {ref[k]:.8g}")
    dist = {}
    for name, g, r in (("cls", grad[..., 4], ref["g_att"]), ("box", grad[..., :4], ref["g_reg"])):
        scale = np.abs(r).max()
        dist[name] = (np.abs(g - r).max(), scale)
        print(f"{tag} {name} gradient: max|gpu - ref| / max|ref| = {dist[name][0] / scale:.3g}  (max|ref| {scale:.4g})")
    for k in SCALARS:
        np.testing.assert_allclose(got[k], ref[k], rtol=LOSS_RTOL, err_msg=f"{tag} {k}")
    for name, (d, scale) in dist.items():
        assert scale > 0 and d <= GRAD_TOL * scale, f"{tag}: {name} gradient off by {d / scale:.3g} of max|ref|"
    assert np.all(grad[..., :4][~ref["mask"]] == 0), f"{tag}: a negative anchor got a box gradient"


def test_inputs_have_several_positives_with_targets_inside_the_unit_interval():
    """on the CPU: what the parity tests below rely on"""
    for A, B in SHAPES:
        for disjoint in (False, True):
            ref = reference(A, B, disjoint, "qfl", "none", True, 2.0, 0.25)
            mask, q = ref["mask"], ref["q"]
            assert np.all(mask.sum(1) > 1)
            assert np.all(q[~mask] == 0)
            inside = q[mask][(q[mask] > 0) & (q[mask] < 1)]
            if disjoint:                                         # (every second positive is moved off the annotation)
                assert inside.size >= 1 and np.any(q[mask] == 0), (A, B, q[mask])     # q = 0: vfl's positive term vanishes, qfl's does not
            else:
                assert inside.size == mask.sum() > 1 and inside.max() - inside.min() > 0.05, (A, B, q[mask])
            assert np.abs(ref["g_att"]).min() > 0                # qfl: every anchor has a live gradient
    ref = reference(315, 3, True, "vfl", "none", True, 2.0, 0.25)
    dead = ref["mask"] & (ref["q"] == 0)
    assert dead.any() and np.all(ref["g_att"][dead] == 0) and np.all(ref["g_att"][~dead] != 0)


@pytest.mark.parametrize("use_multi", [True, False], ids=["multi", "nomulti"])
@pytest.mark.parametrize("box_iou", ["none", "giou"])
@pytest.mark.parametrize("kind", Q.KINDS)
def test_parity_with_fp64_reference(M, kind, box_iou, use_multi):
    for gamma, alpha in GAMMA_ALPHA:
        for A, B in SHAPES:
            for disjoint in (False, True):
                att, reg, annot, anc = inputs(A, B, disjoint)
                ref = reference(A, B, disjoint, kind, box_iou, use_multi, gamma, alpha)
                got, grad, midx, npos = run(M, att, reg, annot, anc, cls_quality=kind, box_iou_loss=box_iou, use_multi=use_multi,
                                            gamma=gamma, alpha=alpha)
                assert ("iou_ls" in got) == (box_iou != "none")
                check(f"{kind} {box_iou} {'multi' if use_multi else 'nomulti'} gamma={gamma} alpha={alpha} A={A} B={B}"
                      f"{' disjoint' if disjoint else ''}", got, grad, ref)
                assert np.array_equal(midx, ref["best"].astype(np.int32)) and np.array_equal(npos, ref["mask"].sum(1).astype(np.int32))


@pytest.mark.parametrize("kind", Q.KINDS)
def test_weights_compose(M, kind):
    """lamb_reg = 0 (no smooth-L1 term) and lamb_iou = 2.5 next to the quality term"""
    for A, B in SHAPES:
        att, reg, annot, anc = inputs(A, B)
        ref = Q.compose(O, att, reg, annot, anc, kind, "diou", lamb_reg=0.0, lamb_iou=2.5)
        got, grad, _, _ = run(M, att, reg, annot, anc, cls_quality=kind, box_iou_loss="diou", lamb_reg=0, lamb_iou=2.5)
        check(f"{kind} diou lamb_reg=0 lamb_iou=2.5 A={A} B={B}", got, grad, ref)
        np.testing.assert_allclose(got["loss"], 2.5 * ref["iou_ls"] + ref["cls_ls"], rtol=LOSS_RTOL)


@pytest.mark.parametrize("use_multi", [True, False], ids=["multi", "nomulti"])
@pytest.mark.parametrize("box_iou", ["none", "giou"])
def test_box_path_and_matching_are_bit_equal_to_the_plain_loss(M, box_iou, use_multi):
    """q is detached and the box path is untouched: the box gradient, box_ls, iou_ls and the matching do not see the quality term"""
    for A, B in SHAPES:
        for disjoint in (False, True):
            att, reg, annot, anc = inputs(A, B, disjoint)
            plain, gradp, midxp, nposp = run(M, att, reg, annot, anc, box_iou_loss=box_iou, use_multi=use_multi)
            assert "pos_iou" not in plain
            pos_iou = []
            for kind in Q.KINDS:
                got, grad, midx, npos = run(M, att, reg, annot, anc, cls_quality=kind, box_iou_loss=box_iou, use_multi=use_multi)
                assert np.array_equal(grad[..., :4].view(np.int32), gradp[..., :4].view(np.int32)), (kind, A, B)
                assert np.abs(gradp[..., :4]).max() > 0
                assert not np.array_equal(grad[..., 4], gradp[..., 4])
                assert np.array_equal(midx, midxp) and np.array_equal(npos, nposp)
                assert got["box_ls"] == plain["box_ls"] and got.get("iou_ls") == plain.get("iou_ls")
                assert got["cls_ls"] != plain["cls_ls"]
                pos_iou.append(got["pos_iou"])
            assert pos_iou[0] == pos_iou[1]


def raw_call(entry, att, reg, annot, anc, flags, scale=1.0, iou_kind=None, cls_kind=None, alpha=0.25, gamma=2.0, lamb_iou=1.5, n=None):
    """one of the three C entry points -> (rc, losses, grad5, match_idx, npos) as numpy"""
    from zsgnet_pytorch_amd._lib import lib, stream_ptr
    B, A = att.shape
    out5 = torch.cat([torch.from_numpy(reg), torch.from_numpy(att)[..., None]], dim=2).cuda().contiguous()
    an, bx = torch.from_numpy(anc).cuda(), torch.from_numpy(annot).cuda()
    n = n or {"zsg_loss_fwd_bwd": 3, "zsg_loss_fwd_bwd_iou": 4, "zsg_loss_fwd_bwd_q": 5}[entry]
    losses, grad = torch.full((n,), -7.0, device="cuda"), torch.full_like(out5, -7.0)
    midx, npos = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    wsb = lib.zsg_loss_workspace_bytes(B, A)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device="cuda")
    head = (out5.data_ptr(), bx.data_ptr(), an.data_ptr(), B, A, alpha, gamma, 1.0, 0.6, flags, scale)
    tail = (losses.data_ptr(), grad.data_ptr(), midx.data_ptr(), npos.data_ptr(), ws.data_ptr(), wsb, stream_ptr())
    mid = {"zsg_loss_fwd_bwd": (), "zsg_loss_fwd_bwd_iou": (iou_kind, lamb_iou), "zsg_loss_fwd_bwd_q": (iou_kind, lamb_iou, cls_kind)}[entry]
    rc = getattr(lib, entry)(*head, *mid, *tail)
    torch.cuda.synchronize()
    return rc, losses.cpu().numpy(), grad.cpu().numpy(), midx.cpu().numpy(), npos.cpu().numpy()


@pytest.mark.parametrize("flags", [3, 1, 2, 0, 5], ids=["focal_multi", "focal", "multi", "plain", "softmax"])
def test_cls_kind_0_equals_the_older_entries_bit_for_bit(M, flags):
    for A, B in [(100, 3), (130, 1), (315, 3)]:
        att, reg, annot, anc = inputs(A, B, True)
        for iou_kind in (0, 1, 2):
            if iou_kind:
                old = raw_call("zsg_loss_fwd_bwd_iou", att, reg, annot, anc, flags, iou_kind=iou_kind)
            else:
                old = raw_call("zsg_loss_fwd_bwd", att, reg, annot, anc, flags)
            new = raw_call("zsg_loss_fwd_bwd_q", att, reg, annot, anc, flags, iou_kind=iou_kind, cls_kind=0)
            assert old[0] == 0 and new[0] == 0
            k = len(old[1])
            assert np.array_equal(new[1][:k].view(np.int32), old[1].view(np.int32)), (A, B, iou_kind, new[1], old[1])
            if not iou_kind:
                assert new[1][3] == 0.0
            assert np.isfinite(new[1][4]) and new[1][4] >= 0
            assert np.array_equal(new[2].view(np.int32), old[2].view(np.int32)), (A, B, iou_kind)
            assert np.array_equal(new[3], old[3]) and np.array_equal(new[4], old[4])


def test_pos_iou_is_the_mean_target_of_the_positives(M):
    """against q computed by the torch reference (decode + IoU written out there; no kernel of the library takes part)"""
    for A, B in SHAPES:
        for disjoint in (False, True):
            att, reg, annot, anc = inputs(A, B, disjoint)
            mask = O.zsg_loss(att, reg, annot, anc)["mask"]
            q = Q.quality_target(reg, annot, anc, mask).numpy()
            want = np.mean([q[b][mask[b]].mean() for b in range(B)])
            rc, losses, _, _, _ = raw_call("zsg_loss_fwd_bwd_q", att, reg, annot, anc, 3, iou_kind=0, cls_kind=1)
            print(f"A={A} B={B}{' disjoint' if disjoint else ''} pos_iou: gpu {losses[4]:.8g} ref {want:.8g}")
            assert rc == 0
            np.testing.assert_allclose(losses[4], want, rtol=LOSS_RTOL)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_two_runs_are_bit_identical(M, kind):
    for A, B in [(100, 3), (315, 3)]:
        att, reg, annot, anc = inputs(A, B, True)
        kw = dict(cls_quality=kind, box_iou_loss="giou", gamma=1.5)
        a, b = run(M, att, reg, annot, anc, **kw), run(M, att, reg, annot, anc, **kw)
        assert a[0] == b[0]
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("cls_kind", [1, 2])
def test_grad_scale_quarters_the_gradient_exactly(M, cls_kind):
    """the raw entry point: grad_scale = 1 / 4 (the 1 / world pre-scaling of four data-parallel ranks) is an exact scaling by a power of two"""
    for A, B in [(100, 3), (315, 3)]:
        att, reg, annot, anc = inputs(A, B)
        res = [raw_call("zsg_loss_fwd_bwd_q", att, reg, annot, anc, 3, scale=s, iou_kind=1, cls_kind=cls_kind) for s in (1.0, 0.25)]
        assert res[0][0] == 0 and res[1][0] == 0
        assert np.array_equal(res[0][1], res[1][1])                       # the loss values are not scaled
        assert np.abs(res[0][2][..., 4]).min() > 0
        assert np.array_equal((res[0][2] * np.float32(0.25)).view(np.int32), res[1][2].view(np.int32))


@pytest.mark.parametrize("box_iou", ["none", "giou"])
@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("A", [100, 315])
def test_nan_rule(M, kind, box_iou, A):
    """a NaN att logit (at a negative and at a positive anchor): the constants, iou_ls = pos_iou = 0, no gradient anywhere"""
    att, reg, annot, anc = inputs(A, 3)
    mask = reference(A, 3, False, kind, "none", True, 2.0, 0.25)["mask"]
    for where in (np.nonzero(~mask[1])[0][-1], np.nonzero(mask[1])[0][-1]):
        bad = att.copy()
        bad[1, where] = float("nan")
        got, grad, _, _ = run(M, bad, reg, annot, anc, cls_quality=kind, box_iou_loss=box_iou)
        assert got["cls_ls"] == 1.0 and got["box_ls"] == np.float32(0.01) and got.get("iou_ls", 0.0) == 0.0 and got["pos_iou"] == 0.0, got
        np.testing.assert_allclose(got["loss"], 1.01, rtol=1e-6)
        assert np.all(grad == 0)


def test_limits_are_rejected(M):
    from zsgnet_pytorch_amd._lib import lib
    A = 100
    att, reg, annot, anc = inputs(A, 3)
    big = [np.ascontiguousarray(np.resize(x, (513,) + x.shape[1:])) for x in (att, reg, annot)]
    rc = raw_call("zsg_loss_fwd_bwd_q", *big, anc, 3, iou_kind=1, cls_kind=1)[0]
    assert rc == -1 and b"513" in lib.zsg_last_error()
    assert raw_call("zsg_loss_fwd_bwd_q", *[x[:512] for x in big], anc, 3, iou_kind=1, cls_kind=1)[0] == 0
    for kw in (dict(cls_kind=3, iou_kind=0), dict(cls_kind=1, iou_kind=3), dict(cls_kind=1, iou_kind=0, gamma=0.5)):
        assert raw_call("zsg_loss_fwd_bwd_q", att, reg, annot, anc, 3, **kw)[0] == -1, kw
    for flags in (2, 5):                                 # no use_focal; use_softmax
        assert raw_call("zsg_loss_fwd_bwd_q", att, reg, annot, anc, flags, iou_kind=0, cls_kind=2)[0] == -1, flags


@pytest.mark.parametrize("kind", Q.KINDS)
def test_full_width(M, gold, kind):
    """A = 17460 (300 x 300), B = 2: the chunked path at the real width"""
    anchors, config, loss = M
    g = gold("g5_loss_eval_full")
    gen = torch.Generator().manual_seed(int(g["gen_seed"][0]))
    att = (torch.randn(2, 17460, generator=gen) * 1.5 - 3.0).numpy()
    reg = (torch.randn(2, 17460, 4, generator=gen) * 0.3).numpy()
    anc = anchors.create_anchors(O.feat_sizes_for(300, 300), RATIOS, SCALES, device="cuda").cpu().numpy()
    assert anc.shape == (17460, 4)
    ref = Q.compose(O, att, reg, g["annot"], anc, kind, "giou")
    got, grad, midx, npos = run(M, att, reg, g["annot"], anc, cls_quality=kind, box_iou_loss="giou")
    print("npos", npos)
    check(f"{kind} giou A=17460 B=2", got, grad, ref)
    assert np.array_equal(midx, ref["best"].astype(np.int32)) and np.array_equal(npos, ref["mask"].sum(1).astype(np.int32))

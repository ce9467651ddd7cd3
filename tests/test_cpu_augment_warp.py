"""Box-aware rotation / shear and Gaussian blur of the training augmentation, on the host: steps 6 and 7 of dat_loader.augment_host pinned
by checks that do not reuse its code path (np.rot90, explicit shifts, impulse responses, painted rectangles), dat_loader.warp_matrix /
warp_box / settle_warp / blur_taps, dat_loader.draw_augment_warp (draw order, the unchanged random stream with the new keys off), cfg
validation and the loader plumbing.  The HIP kernels (zsg_augment_warp_u8_batched) are measured against augment_host in
tests/test_gpu_augment_warp.py."""
import math
import os

import numpy as np
import pytest
import torch

import test_cpu_augment as T0
import test_cpu_augment_geom as T1
from zsgnet_pytorch_amd import config, dat_loader as D

ROOT = T0.ROOT
AUG, back_to_image = T0.AUG, T0.back_to_image
tiny = T0.tiny                                   # the fixture: three PNGs, a five-row CSV, a word-vector table
FILL = (124, 116, 104)
ONES = np.ones(3, np.float32)
WARP = dict(aug_rotate=15.0, aug_shear=8.0, aug_blur=2.0)
ITEM_KEYS = {"img", "idxs", "qvec", "qlens", "annot", "orig_annot", "img_size"}
ROT = {90: (0, 65536, None, -65536, 0, None), 180: (-65536, 0, None, 0, -65536, None), 270: (0, -65536, None, 65536, 0, None)}


def rot_matrix(deg, n):
    """the explicit 16.16 inverse map of a rotation by 90 / 180 / 270 degrees of an n x n image: the source pixel of output (x, y) is
    (y, n - 1 - x) / (n - 1 - x, n - 1 - y) / (n - 1 - y, x)"""
    a, b, _, d, e, _ = ROT[deg]
    c0 = {90: 0, 180: n - 1, 270: n - 1}[deg] * 65536
    c1 = {90: n - 1, 180: n - 1, 270: 0}[deg] * 65536
    return a, b, c0, d, e, c1


def whole(a):
    return (0, 0, a.shape[1], a.shape[0])


def warped(a, m, fill=FILL, blur=0.0):
    """augment_host of an image at its own size with factors 1: steps 1-5 are the identity (Pillow skips a pass that keeps the length)"""
    return D.augment_host(a, whole(a), ONES, a.shape[:2], fill=fill, warp=m, blur=blur)


# ---- 1. the warp ----------------------------------------------------------------------------------------------------------------------------
def test_identity_and_right_angle_rotations_are_exact():
    rng = np.random.RandomState(0)
    for hw in ((9, 9), (16, 16), (25, 31), (40, 48)):
        a = rng.randint(0, 256, (*hw, 3)).astype(np.uint8)
        assert D.warp_matrix(0.0, 0.0, hw) == (65536, 0, 0, 0, 65536, 0) == D.WARP_IDENTITY
        assert np.array_equal(D.warp_host(a, D.WARP_IDENTITY, FILL), a) and np.array_equal(warped(a, D.WARP_IDENTITY), a)
        assert np.array_equal(warped(a, None), a)
    for n in (9, 16):
        a = rng.randint(0, 256, (n, n, 3)).astype(np.uint8)
        for deg, k in ((90, 3), (180, 2), (270, 1)):
            assert np.array_equal(warped(a, rot_matrix(deg, n), fill=(1, 2, 3)), np.rot90(a, k)), (n, deg)
            assert D.warp_matrix(float(deg), 0.0, (n, n)) == rot_matrix(deg, n), "a positive theta turns the picture clockwise on screen"


def test_integer_translation_is_a_shift_with_fill():
    rng = np.random.RandomState(1)
    for hw in ((9, 9), (25, 31)):
        a = rng.randint(0, 256, (*hw, 3)).astype(np.uint8)
        h, w = hw
        out = warped(a, (65536, 0, -2 * 65536, 0, 65536, 3 * 65536), fill=(7, 8, 9))      # output (x, y) <- source (x - 2, y + 3)
        exp = np.empty_like(a)
        exp[:] = (7, 8, 9)
        exp[0:h - 3, 2:w] = a[3:h, 0:w - 2]
        assert np.array_equal(out, exp)
        # half a pixel to the right: the rounded mean of horizontal neighbours, the last column blends with the fill
        out = warped(a, (65536, 0, 32768, 0, 65536, 0), fill=(0, 0, 0))
        nxt = np.concatenate([a[:, 1:], np.zeros((h, 1, 3), np.uint8)], 1).astype(np.int64)
        assert np.array_equal(out, ((a.astype(np.int64) + nxt) * 128 * 256 + 32768 >> 16).astype(np.uint8))
    with pytest.raises(ValueError, match="fill"):
        D.augment_host(a, whole(a), ONES, a.shape[:2], warp=(65536, 0, 65536, 0, 65536, 0))


def box_of_pixels(out):
    ys, xs = np.nonzero(out[..., 0] >= 128)
    return xs.min(), ys.min(), xs.max() + 1, ys.max() + 1


def test_pixels_and_boxes_move_the_same_way():
    """a white rectangle on black, warped: the bounding box of its bright pixels lies within 1.0 output pixel of warp_box's result on
    every side (a sign or direction error moves a side by many pixels; sampling and the >= 128 threshold account for < 1)"""
    rng = np.random.RandomState(2)
    worst = 0.0
    for trial in range(300):
        Ho, Wo = [(40, 48), (25, 31), (64, 64)][trial % 3]
        th, sh = rng.uniform(-15, 15), rng.uniform(-8, 8)
        x1, x2 = rng.uniform(0.3 * Wo, 0.45 * Wo), rng.uniform(0.55 * Wo, 0.7 * Wo)
        y1, y2 = rng.uniform(0.3 * Ho, 0.45 * Ho), rng.uniform(0.55 * Ho, 0.7 * Ho)
        bx = tuple(int(round(v)) for v in (x1, y1, x2, y2))
        im = np.zeros((Ho, Wo, 3), np.uint8)
        im[bx[1]:bx[3], bx[0]:bx[2]] = 255
        out = warped(im, D.warp_matrix(th, sh, (Ho, Wo)), fill=(0, 0, 0))
        want = D.warp_box(bx, th, sh, (Ho, Wo), (Ho, Wo))                                  # window == output: window pixels are output pixels
        assert 0 < want[0] and 0 < want[1] and want[2] < Wo and want[3] < Ho, "nothing is clipped here: the result is the unclipped box"
        dev = max(abs(g - e) for g, e in zip(box_of_pixels(out), want))
        worst = max(worst, dev)
        assert dev <= 1.0, (trial, (Ho, Wo), th, sh, bx, box_of_pixels(out), want)
    print(f"rectangle against warp_box: worst side deviation {worst:.3f} output pixels over 300 draws")
    # the signs, each alone: theta > 0 is clockwise on screen (the top edge's right end goes down), shear > 0 moves the bottom to the right
    im = np.zeros((64, 64, 3), np.uint8)
    im[30:34, 8:56] = 255                                                                  # a horizontal bar through the centre
    out = warped(im, D.warp_matrix(15.0, 0.0, (64, 64)), fill=(0, 0, 0))
    ys, xs = np.nonzero(out[..., 0] >= 128)
    assert ys[xs > 48].mean() > 32 + 4 and ys[xs < 16].mean() < 32 - 4
    im = np.zeros((64, 64, 3), np.uint8)
    im[8:56, 30:34] = 255                                                                  # a vertical bar
    out = warped(im, D.warp_matrix(0.0, 8.0, (64, 64)), fill=(0, 0, 0))
    ys, xs = np.nonzero(out[..., 0] >= 128)
    assert xs[ys > 48].mean() > 32 + 1.5 and xs[ys < 16].mean() < 32 - 1.5
    # a window that is not the output: the box is scaled to output pixels, warped there, and scaled back
    got = D.warp_box((10, 5, 30, 25), 10.0, 4.0, (40, 48), (80, 24))
    ref = D.warp_box((20, 2.5, 60, 12.5), 10.0, 4.0, (40, 48), (40, 48))
    assert np.allclose(got, np.array(ref) * [0.5, 2, 0.5, 2], atol=1e-9)


# ---- 2. the blur ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 0.3, 0.5, 1.0, 2.0, 2.5])
def test_blur_taps_and_impulse_response(sigma):
    r, t = D.blur_taps(sigma)
    assert r == min(8, math.ceil(3 * sigma)) and len(t) == 2 * r + 1
    assert int(t.sum()) == 65536 and (t >= 0).all() and np.array_equal(t, t[::-1]) and t[r] == t.max()
    w = np.exp(-np.arange(-r, r + 1) ** 2 / (2 * sigma ** 2))
    assert np.abs(t / 65536.0 - w / w.sum()).max() < 2.0 / 65536 * (2 * r + 1)            # every tap rounded, the centre takes the rest
    cst = np.full((11, 13, 3), 201, np.uint8)
    assert np.array_equal(D.blur_host(cst, sigma), cst) and np.array_equal(warped(cst, None, blur=sigma), cst)
    # an impulse in the middle of a line: the response along each axis is the tap table (tap * 255, rounded as defined)
    resp = (t * 255 + 32768) >> 16
    n = 2 * r + 5
    row = np.zeros((1, n, 3), np.uint8)
    row[0, n // 2] = 255
    assert D.blur_host(row, sigma)[0, n // 2 - r:n // 2 + r + 1, 1].tolist() == resp.tolist()      # (height 1: the clamped vertical pass keeps it)
    col = np.zeros((n, 1, 3), np.uint8)
    col[n // 2, 0] = 255
    assert D.blur_host(col, sigma)[n // 2 - r:n // 2 + r + 1, 0, 2].tolist() == resp.tolist()
    # the border is clamped: an impulse in the corner pixel collects the taps that fall outside
    row = np.zeros((1, n, 3), np.uint8)
    row[0, 0] = 255
    assert int(D.blur_host(row, sigma)[0, 0, 0]) == (int(t[:r + 1].sum()) * 255 + 32768) >> 16


def test_blur_taps_reject_bad_sigmas():
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            D.blur_taps(bad)
    assert D.blur_taps(10.0)[0] == 8, "the radius is capped at 8"


# ---- 3. the box rule ------------------------------------------------------------------------------------------------------------------------
def kept_fraction(box, th, sh, out_hw):
    """the rule restated: the corners through M = R S by hand, the clipped over the unclipped area"""
    Ho, Wo = out_hw
    t, s = math.radians(th), math.radians(sh)
    R = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    S = np.array([[1.0, math.tan(s)], [0.0, 1.0]])
    c = np.array([Wo / 2.0, Ho / 2.0])
    P = np.array([[box[0], box[1]], [box[2], box[1]], [box[0], box[3]], [box[2], box[3]]], float)
    Q = ((R @ S) @ (P - c).T).T + c
    x1, y1, x2, y2 = Q[:, 0].min(), Q[:, 1].min(), Q[:, 0].max(), Q[:, 1].max()
    inside = max(min(x2, Wo) - max(x1, 0), 0) * max(min(y2, Ho) - max(y1, 0), 0)
    return inside / ((x2 - x1) * (y2 - y1)), (max(x1, 0), max(y1, 0), min(x2, Wo), min(y2, Ho))


def test_box_rule():
    rng = np.random.RandomState(3)
    for trial in range(3000):                                                              # boxes inside the central half are never halved
        Ho, Wo = [(300, 300), (24, 32), (40, 30)][trial % 3]
        xs, ys = np.sort(rng.uniform(0.25 * Wo, 0.75 * Wo, 2)), np.sort(rng.uniform(0.25 * Ho, 0.75 * Ho, 2))
        th, sh = rng.uniform(-10, 10), rng.uniform(-5, 5)
        assert D.settle_warp(th, sh, [(xs[0], ys[0], xs[1], ys[1])], (Ho, Wo), (Ho, Wo), 0.8) == (th, sh)
    halved = [0, 0]
    for trial in range(2000):                                                              # border boxes never fall back to identity
        th, sh = rng.uniform(-15, 15), rng.uniform(-8, 8)
        left = (0.0, rng.uniform(0, 100), rng.uniform(50, 300), rng.uniform(150, 300))
        for n, boxes in enumerate(([left], [(0.0, 0.0, 300.0, 300.0)], [left, (0.0, 0.0, 300.0, 300.0)])):
            got = D.settle_warp(th, sh, boxes, (300, 300), (300, 300), 0.8)
            assert got is not None, (th, sh, boxes)
            k = round(math.log2(th / got[0]))
            assert 0 <= k <= 4 and got == (th / 2 ** k, sh / 2 ** k), "both halved together"
            halved[min(n, 1)] += k > 0
            for b in boxes:                                                                # every settled draw keeps every box
                frac, clipped = kept_fraction(b, *got, (300, 300))
                assert frac >= 0.8 - 1e-12
                assert np.allclose(D.warp_box(b, *got, (300, 300), (300, 300), 0.8), clipped, atol=1e-9)
            if k > 0:                                                                      # ... and the draw before the last halving did not
                assert any(kept_fraction(b, 2 * got[0], 2 * got[1], (300, 300))[0] < 0.8 for b in boxes)
    assert halved[0] > 0 and halved[1] > halved[0]
    # a box the rule can never keep (mostly outside already): four halvings, then the warp is dropped
    assert D.settle_warp(8.0, 2.0, [(-200.0, 10.0, 20.0, 60.0)], (300, 300), (300, 300), 0.8) is None
    assert D.warp_box((-200.0, 10.0, 20.0, 60.0), 0.5, 0.125, (300, 300), (300, 300), 0.8) is None
    assert D.warp_box((-200.0, 10.0, 20.0, 60.0), 0.0, 0.0, (300, 300), (300, 300)) == (0.0, 10.0, 20.0, 60.0), "keep = None: clipped, never refused"
    # keep = 1: only a warp that leaves every box wholly inside
    assert D.settle_warp(10.0, 0.0, [(100.0, 100.0, 200.0, 200.0)], (300, 300), (300, 300), 1.0) == (10.0, 0.0)
    assert D.settle_warp(1.0, 0.0, [(0.0, 0.0, 300.0, 300.0)], (300, 300), (300, 300), 1.0) is None


# ---- 4. the draw ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_kw", [AUG, {}, dict(aug_flip=0.5, aug_expand_max=2.0), dict(**AUG, aug_flip=0.5, aug_expand_max=2.5)])
def test_new_keys_off_is_draw_augment_geom_and_its_random_stream(cfg_kw):
    cfg = config.get_cfg(**cfg_kw)
    for hw in ((37, 53), (64, 48)):
        for name, boxes in T0.box_cases(*hw).items():
            r0, r1 = np.random.RandomState(4), np.random.RandomState(4)
            for _ in range(50):
                old, new = D.draw_augment_geom(r0, *hw, boxes, cfg), D.draw_augment_warp(r1, *hw, boxes, cfg, (40, 48))
                if old is None:
                    assert new is None
                else:
                    assert new[0] == old[0] and np.array_equal(new[1], old[1]) and new[2] is old[2] and new[3] is None and new[4] is None, name
            s0, s1 = r0.get_state(), r1.get_state()
            assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:], "the generator is left in the same state"
    assert D.draw_augment_warp(np.random.RandomState(0), 37, 53, [[1, 2, 3, 4]], {}, (40, 48)) is None      # a cfg without the keys = the defaults


@pytest.mark.parametrize("base", [{}, AUG, dict(**AUG, aug_flip=0.5, aug_expand_max=2.5)])
def test_draw_order_with_the_new_keys_on(base):
    hw, out_hw, boxes = (37, 53), (40, 48), [[14.0, 11.0, 30.0, 25.0]]
    cfg_old = config.get_cfg(**base)
    for new_kw, tail in ((dict(aug_rotate=15.0), ["theta"]), (dict(aug_shear=8.0), ["phi"]), (dict(aug_blur=2.0), ["u", "sigma"]),
                         (dict(aug_rotate=15.0, aug_shear=8.0, aug_blur=2.0, aug_blur_p=0.5), ["theta", "phi", "u", "sigma"])):
        cfg = config.get_cfg(**base, **new_kw)
        applied = {"warp": 0, "blur": 0}
        for seed in range(40):
            rec, r0 = T1.Recorder(seed), T1.Recorder(seed)
            crop, jit, flip, warp, sigma = D.draw_augment_warp(rec, *hw, boxes, cfg, out_hw)
            old = D.draw_augment_geom(r0, *hw, boxes, cfg_old)
            n0 = len(r0.log)
            assert rec.log[:n0] == r0.log, "the first numbers drawn are draw_augment_geom's"
            if old is None:
                assert crop == (0, 0, 53, 37) and jit.tolist() == [1.0, 1.0, 1.0] and flip is False and n0 == 0
            else:
                assert crop == old[0] and np.array_equal(jit, old[1]) and flip is old[2]
            rest = rec.log[n0:]
            assert [k for k, _, _ in rest] == ["uniform"] * len(tail)
            vals = dict(zip(tail, rest))
            if "theta" in vals:
                assert vals["theta"][1] == (-15.0, 15.0)
            if "phi" in vals:
                assert vals["phi"][1] == (-8.0, 8.0)
            if "theta" in vals or "phi" in vals:
                th, ph = vals.get("theta", (0, 0, 0.0))[2], vals.get("phi", (0, 0, 0.0))[2]
                x0, y0, x1, y1 = crop
                b = np.array(boxes[0]) - [x0, y0, x0, y0]
                if flip:
                    b = np.array([x1 - x0 - b[2], b[1], x1 - x0 - b[0], b[3]])
                assert warp == D.settle_warp(th, ph, [b.tolist()], out_hw, (y1 - y0, x1 - x0), 0.8)
                applied["warp"] += warp is not None
            else:
                assert warp is None
            if "u" in vals:
                assert vals["u"][1] == () and vals["sigma"][1] == (0.1, 2.0)
                assert sigma == (float(np.float32(vals["sigma"][2])) if vals["u"][2] < 0.5 else None)
                applied["blur"] += sigma is not None
            else:
                assert sigma is None
        assert applied["warp"] > 20 or "theta" not in tail and "phi" not in tail
        assert 8 < applied["blur"] < 32 or "u" not in tail
    always, never = config.get_cfg(aug_blur=0.1, aug_blur_p=1.0), config.get_cfg(aug_blur=1.0, aug_blur_p=0.0)
    rng = np.random.RandomState(0)
    assert all(D.draw_augment_warp(rng, *hw, boxes, always, out_hw)[4] == float(np.float32(0.1)) for _ in range(20))
    assert all(D.draw_augment_warp(rng, *hw, boxes, never, out_hw)[4] is None for _ in range(20))


# ---- 5. cfg -----------------------------------------------------------------------------------------------------------------------------------
def test_interface_and_errors(tiny):
    g, kw, root = tiny
    from zsgnet_pytorch_amd import _lib as L
    assert "zsg_augment_warp_u8_batched" in open(os.path.join(ROOT, "include", "zsg.h")).read()
    assert "zsg_augment_warp_u8_batched" in L.SIGNATURES and hasattr(L.lib, "zsg_augment_warp_u8_batched")
    assert len(L.SIGNATURES["zsg_augment_warp_u8_batched"][1]) == 8
    c = config.get_cfg()
    assert (c["aug_rotate"], c["aug_shear"], c["aug_warp_keep"], c["aug_blur"], c["aug_blur_p"]) == (0.0, 0.0, 0.8, 0.0, 0.5)
    assert not D.aug_enabled(c) and not D.aug_enabled({})
    for on in (dict(aug_rotate=5.0), dict(aug_shear=3.0), dict(aug_blur=1.0)):
        assert D.aug_enabled(config.get_cfg(**on)) and D.aug_warp_enabled(config.get_cfg(**on))
    assert not D.aug_warp_enabled(config.get_cfg(aug_warp_keep=0.5, aug_blur_p=1.0)), "the two dependent keys switch nothing on"
    for key, bad in (("aug_rotate", -0.1), ("aug_rotate", 30.5), ("aug_rotate", float("nan")), ("aug_shear", -1.0), ("aug_shear", 20.5),
                     ("aug_shear", float("inf")), ("aug_warp_keep", 0.0), ("aug_warp_keep", 1.01), ("aug_warp_keep", -0.5), ("aug_blur", 0.05),
                     ("aug_blur", 2.6), ("aug_blur", -1.0), ("aug_blur", float("nan")), ("aug_blur_p", -0.1), ("aug_blur_p", 1.1)):
        with pytest.raises(ValueError, match=key):
            D.get_data(config.get_cfg(**kw, **{key: bad}), prefetch=False)
    D.get_data(config.get_cfg(**kw, aug_rotate=30.0, aug_shear=20.0, aug_warp_keep=1.0, aug_blur=2.5, aug_blur_p=1.0), prefetch=False)      # the ends are valid
    D.get_data(config.get_cfg(**kw, aug_blur=0.1, aug_blur_p=0.0), prefetch=False)
    from zsgnet_pytorch_amd.main_dist import learner_init
    for on in (dict(aug_rotate=5.0), dict(aug_shear=5.0), dict(aug_blur=1.0)):
        with pytest.raises(ValueError, match="synthetic"):
            learner_init("x", config.get_cfg(synthetic=True, **on))


# ---- 6. the dataset ---------------------------------------------------------------------------------------------------------------------------
def expected_box(box, crop, flip, warp, out_hw):
    """the box rule of the documentation, by hand: window pixels, mirror, then warp_box when a warp applies"""
    x0, y0, x1, y1 = crop
    b = np.asarray(box, np.float64) - np.array([x0, y0, x0, y0])
    if flip:
        b = np.array([x1 - x0 - b[2], b[1], x1 - x0 - b[0], b[3]])
    if warp is not None:
        b = np.array(kept_fraction(b * np.array([out_hw[1] / (x1 - x0), out_hw[0] / (y1 - y0)] * 2), *warp, out_hw)[1]) \
            / np.array([out_hw[1] / (x1 - x0), out_hw[0] / (y1 - y0)] * 2)
    return b


@pytest.mark.parametrize("base", [{}, dict(**AUG, aug_flip=0.5, aug_expand_max=2.0)], ids=["warp keys alone", "every key"])
def test_dataset_items_with_warp_and_blur(tiny, base):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **base, **WARP)
    out_hw = (40, 48)
    raw = {k: g["png_" + k] for k in "abc"}
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)
    ds_h = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train")
    seen = {"warp": 0, "nowarp": 0, "blur": 0, "noblur": 0}
    for rep in range(6):
        for i in range(5):
            np.random.seed(100 * rep + i)
            it = ds_g[i]
            np.random.seed(100 * rep + i)
            ih = ds_h[i]
            im = raw[str(g["csv_img"][i])[0]]
            np.random.seed(100 * rep + i)
            crop, jit, flip, warp, sigma = D.draw_augment_warp(np.random, im.shape[0], im.shape[1], [g["csv_bbox"][i].tolist()], cfg, out_hw)
            assert set(ih) == ITEM_KEYS and set(it) == ITEM_KEYS | {"aug_crop", "aug_jitter", "aug_geom", "aug_warp", "aug_blur"}
            assert it["aug_warp"].dtype == torch.int32 and tuple(it["aug_warp"].shape) == (6,) and it["aug_blur"].dtype == torch.float32 and it["aug_blur"].dim() == 0
            assert it["aug_crop"].tolist() == list(crop) and bool(it["aug_geom"][0]) == flip and it["aug_geom"][1:].tolist() == list(FILL)
            m = tuple(it["aug_warp"].tolist())
            assert m == (D.warp_matrix(*warp, out_hw) if warp is not None else D.WARP_IDENTITY)
            assert float(it["aug_blur"]) == (sigma or 0.0)
            seen["warp" if warp is not None else "nowarp"] += 1
            seen["blur" if sigma else "noblur"] += 1
            assert np.array_equal(it["img"].numpy(), im), "the raw image travels"
            x0, y0, x1, y1 = crop
            assert it["img_size"].tolist() == [y1 - y0, x1 - x0], "img_size stays the window's"
            for k in ("annot", "orig_annot", "img_size", "qvec", "qlens", "idxs"):
                assert torch.equal(it[k], ih[k]), k
            box = expected_box(g["csv_bbox"][i], crop, flip, warp, out_hw)
            assert np.abs(it["orig_annot"].double().numpy() - box).max() < 1e-3
            assert np.abs(back_to_image(it["annot"], (0, 0, x1 - x0, y1 - y0)) - it["orig_annot"].double().numpy()).max() < 1e-3
            # the worker path's image: augment_host of the raw image with the drawn warp and blur (sigma as the item carries it: float32)
            want = D.augment_host(im, crop, jit, out_hw, flip=flip, fill=FILL, warp=m, blur=float(sigma or 0.0))
            assert torch.equal(ih["img"], torch.from_numpy(want.transpose(2, 0, 1).astype(np.float64)).float().div_(255))
            if warp is not None or sigma:
                plain = D.augment_host(im, crop, jit, out_hw, flip=flip, fill=FILL)
                assert not np.array_equal(want, plain), "the warp / blur changes the image"
    assert seen["warp"] > 10 and seen["blur"] > 5 and seen["noblur"] > 5
    b = D.collater([ds_g[0], ds_g[2]])
    assert b["aug_warp"].dtype == torch.int32 and tuple(b["aug_warp"].shape) == (2, 6) and b["aug_blur"].dtype == torch.float32 and tuple(b["aug_blur"].shape) == (2,)


def test_the_drawn_sigma_is_the_float32_the_item_carries(tiny):
    """aug_blur travels as float32, so the draw rounds sigma to float32 once: the worker path and the GPU path build the same taps"""
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, aug_blur=2.5, aug_blur_p=1.0)
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)
    for seed in range(50):
        np.random.seed(seed)
        s32 = float(ds_g[seed % 5]["aug_blur"])
        np.random.seed(seed)
        s64 = D.draw_augment_warp(np.random, 30, 40, [[1, 2, 3, 4]], cfg, (40, 48))[4]
        assert s32 == s64 and 0.1 <= s64 <= 2.5 + 1e-6


def test_grouped_training_batch_warps_a_slot_together(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG, aug_flip=0.5, **WARP)
    out_hw = (40, 48)
    chunks, rows = [[0, 3], [2, 4]], [0, 3, 2, 4]
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)
    ds_h = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train")
    warped_slots = 0
    for seed in range(8):
        np.random.seed(seed)
        b = ds_g.grouped_train_batch(chunks)
        np.random.seed(seed)
        bh = ds_h.grouped_train_batch(chunks)
        np.random.seed(seed)
        draws = [D.draw_augment_warp(np.random, *g["png_" + k].shape[:2], [g["csv_bbox"][r].tolist() for r in ch], cfg, out_hw) for k, ch in zip("ac", chunks)]
        assert b["aug_warp"].dtype == torch.int32 and tuple(b["aug_warp"].shape) == (2, 6) and tuple(b["aug_blur"].shape) == (2,) and tuple(b["aug_geom"].shape) == (2, 4)
        assert not any(k.startswith("aug_") for k in bh) and tuple(bh["img"].shape) == (2, 3, 40, 48)
        for k in ("annot", "orig_annot", "img_size", "qvec", "qlens"):
            assert torch.equal(b[k], bh[k]), k
        for q, row in enumerate(rows):
            s = int(b["img_idx"][q])
            crop, jit, flip, warp, sigma = draws[s]
            box = expected_box(g["csv_bbox"][row], crop, flip, warp, out_hw)
            assert np.abs(b["orig_annot"][q].double().numpy() - box).max() < 1e-3, "every query of a slot is warped with the slot"
            assert b["img_size"][q].tolist() == [crop[3] - crop[1], crop[2] - crop[0]]
            assert np.abs(back_to_image(b["annot"][q], (0, 0, crop[2] - crop[0], crop[3] - crop[1])) - b["orig_annot"][q].double().numpy()).max() < 1e-3
        for s, k in enumerate("ac"):
            crop, jit, flip, warp, sigma = draws[s]
            warped_slots += warp is not None
            assert tuple(b["aug_warp"][s].tolist()) == (D.warp_matrix(*warp, out_hw) if warp is not None else D.WARP_IDENTITY)
            if warp is not None:                                                           # the settled draw keeps EVERY box of the slot
                for r in chunks[s]:
                    bx = expected_box(g["csv_bbox"][r], crop, flip, None, out_hw)
                    assert D.warp_box(bx, *warp, out_hw, (crop[3] - crop[1], crop[2] - crop[0]), 0.8) is not None
            want = D.augment_host(g["png_" + k], crop, jit, out_hw, flip=flip, fill=FILL, warp=b["aug_warp"][s].tolist(), blur=float(sigma or 0.0))
            assert torch.equal(bh["img"][s], torch.from_numpy(want.transpose(2, 0, 1).astype(np.float64)).float().div_(255))
    assert warped_slots > 8
    assert not any(k.startswith("aug_") for k in ds_g.grouped_batch([0, 3, 2]))            # the grouped VALIDATION batch is never augmented


def test_validation_is_the_golden_and_old_configurations_keep_their_fields(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG, **WARP)
    data = D.get_data(cfg, prefetch=False)
    assert data.train_dl.dataset.augment and data.train_dl.dataset.aug_warp and not data.valid_dl.dataset.augment and not data.valid_dl.dataset.aug_warp
    np.random.seed(0)
    tr = list(data.train_dl)
    assert len(tr) == 1 and not any(k.startswith("aug_") for k in tr[0])
    dv = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "valid")
    for i in range(5):
        it = dv[i]
        assert set(it) == ITEM_KEYS
        for k, v in it.items():
            assert np.array_equal(v.numpy(), g[f"item{i}_{k}"]), (i, k)
    d_old = D.ImgQuDataset(config.get_cfg(**kw, **AUG), root / "d.csv", "refclef", "train", gpu_resize=True)
    assert not d_old.aug_warp and d_old.aug_fill is None and set(d_old[0]) == ITEM_KEYS | {"aug_crop", "aug_jitter"}
    d_geom = D.ImgQuDataset(config.get_cfg(**kw, aug_flip=0.5), root / "d.csv", "refclef", "train", gpu_resize=True)
    assert not d_geom.aug_warp and set(d_geom[0]) == ITEM_KEYS | {"aug_crop", "aug_jitter", "aug_geom"}

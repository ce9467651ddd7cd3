"""Zoom-out and phrase-aware horizontal flip of the training augmentation, on the host: dat_loader.augment_host(..., flip, fill) against
Pillow (a filled canvas, paste, crop, resize, FLIP_LEFT_RIGHT) and against the function without the new keywords (pinned by
tests/test_cpu_augment.py) applied to the materialised canvas; dat_loader.draw_augment_geom (draw order, invariants, the unchanged
random stream with the new keys off); the mirrored box and the swapped direction words; the loader plumbing and cfg validation.
The HIP kernels (zsg_augment_geom_u8_batched) are measured against augment_host in tests/test_gpu_augment_geom.py."""
import os

import numpy as np
import pytest
import torch

import test_cpu_augment as T0
from zsgnet_pytorch_amd import config, dat_loader as D

ROOT = T0.ROOT
AUG, TRIPLES, images, box_cases, back_to_image = T0.AUG, T0.TRIPLES, T0.images, T0.box_cases, T0.back_to_image
tiny = T0.tiny                                   # the fixture: three PNGs, a five-row CSV, a word-vector table
OUTS = T0.OUTS + [(25, 31)]                      # (Ho, Wo)
FILL = (124, 116, 104)
GEOM = dict(aug_flip=0.5, aug_expand_max=2.5)
ITEM_KEYS = {"img", "idxs", "qvec", "qlens", "annot", "orig_annot", "img_size"}


def windows(h, w, out_hw):
    """inside | overhang left + top | right + bottom | all four sides | 3x the image, off-centre | one image pixel in the window's corner
    (top-left, then bottom-right) | window sides == output sides with overhang (Pillow skips both passes) | width == output width only"""
    Ho, Wo = out_hw
    return [(2, 3, 15, 13), (-5, -4, w - 3, h - 2), (4, 3, w + 7, h + 6), (-3, -2, w + 5, h + 4), (-w - 5, -(h // 2), 2 * w - 5, 3 * h - h // 2),
            (w - 1, h - 1, w + 19, h + 16), (-18, -21, 1, 1), (-3, -2, Wo - 3, Ho - 2), (w - 9, 1, w - 9 + Wo, h - 1)]


def canvas_of(a, win, fill):
    """(the image pasted on a fill-coloured canvas that covers the window, the window in canvas coordinates), made by Pillow"""
    import PIL.Image
    h, w = a.shape[:2]
    x0, y0, x1, y1 = win
    cx0, cy0, cx1, cy1 = min(x0, 0), min(y0, 0), max(x1, w), max(y1, h)
    cv = PIL.Image.new("RGB", (cx1 - cx0, cy1 - cy0), tuple(fill))
    cv.paste(PIL.Image.fromarray(a), (-cx0, -cy0))
    return cv, (x0 - cx0, y0 - cy0, x1 - cx0, y1 - cy0)


# ---- 1. the definition --------------------------------------------------------------------------------------------------------------------
def test_augment_host_with_fill_and_flip_is_pillow(gold):
    import PIL.Image
    ones = np.ones(3, np.float32)
    for n, a in enumerate(images(gold)):
        h, w = a.shape[:2]
        for out_hw in OUTS:
            Ho, Wo = out_hw
            for win in windows(h, w, out_hw):
                fill = FILL if n % 2 == 0 else (0, 255, 7)
                cv, cwin = canvas_of(a, win, fill)
                ref = cv.crop(cwin).resize((Wo, Ho))
                got = D.augment_host(a, win, ones, out_hw, fill=fill)
                assert got.dtype == np.uint8 and got.shape == (Ho, Wo, 3)
                assert np.array_equal(got, np.asarray(ref)), f"image {n} {(h, w)} window {win} -> {out_hw}: differs from Pillow's canvas crop().resize()"
                flipped = D.augment_host(a, win, ones, out_hw, flip=True, fill=fill)
                assert flipped.flags["C_CONTIGUOUS"]
                assert np.array_equal(flipped, np.asarray(ref.transpose(PIL.Image.FLIP_LEFT_RIGHT))), f"image {n} window {win} -> {out_hw}, flipped"
            # an inside window: the fill is never seen, and a flip without fill is the mirrored result of today's function
            inside = (1, 2, w - 3, h - 1)
            today = D.augment_host(a, inside, ones, out_hw)
            assert np.array_equal(D.augment_host(a, inside, ones, out_hw, fill=(9, 9, 9)), today)
            assert np.array_equal(D.augment_host(a, inside, ones, out_hw, flip=True), today[:, ::-1])


def test_augment_host_with_factors_is_the_pinned_function_on_the_canvas(gold):
    for n, a in enumerate(images(gold)):
        h, w = a.shape[:2]
        out_hw = OUTS[n % 3]
        for win in (windows(h, w, out_hw)[3], windows(h, w, out_hw)[4 + n % 2]):
            cv, cwin = canvas_of(a, win, FILL)
            cv = np.asarray(cv)
            for t in TRIPLES:
                t = np.array(t, np.float32)
                ref = D.augment_host(cv, cwin, t, out_hw)                              # an inside window of the materialised canvas
                assert np.array_equal(D.augment_host(a, win, t, out_hw, fill=FILL), ref), f"image {n} window {win} factors {t}"
                assert np.array_equal(D.augment_host(a, win, t, out_hw, flip=True, fill=FILL), ref[:, ::-1]), f"image {n} window {win} factors {t}, flipped"


# ---- 2. the draw ------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """numpy's uniform / randint interface of a RandomState, every call and its result written down"""

    def __init__(self, seed):
        self.rng, self.log = np.random.RandomState(seed), []

    def uniform(self, *a):
        v = self.rng.uniform(*a)
        self.log.append(("uniform", a, v))
        return v

    def randint(self, *a):
        v = self.rng.randint(*a)
        self.log.append(("randint", a, v))
        return v


@pytest.mark.parametrize("cfg_kw", [AUG, {}, dict(aug_contrast=0.5), dict(aug_crop_min=0.5)])
def test_new_keys_off_is_draw_augment_and_its_random_stream(cfg_kw):
    cfg = config.get_cfg(**cfg_kw)
    for hw in ((37, 53), (64, 48)):
        for name, boxes in box_cases(*hw).items():
            r0, r1 = np.random.RandomState(4), np.random.RandomState(4)
            for _ in range(50):
                old, new = D.draw_augment(r0, *hw, boxes, cfg), D.draw_augment_geom(r1, *hw, boxes, cfg)
                if old is None:
                    assert new is None
                else:
                    assert new[0] == old[0] and np.array_equal(new[1], old[1]) and new[1].dtype == np.float32 and new[2] is False, name
            s0, s1 = r0.get_state(), r1.get_state()
            assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:], "the generator is left in the same state"
    assert D.draw_augment_geom(np.random.RandomState(0), 37, 53, [[1, 2, 3, 4]], {}) is None      # a cfg without the keys = the defaults


@pytest.mark.parametrize("hw", [(37, 53), (64, 48)])
@pytest.mark.parametrize("crop_on", [True, False])
def test_draw_augment_geom_invariants(hw, crop_on):
    h, w = hw
    emax = 3.0
    cfg = config.get_cfg(**(AUG if crop_on else dict(aug_brightness=0.3)), aug_expand_max=emax, aug_flip=0.5)
    for name, boxes in box_cases(h, w).items():
        rec = Recorder(11)
        b = np.asarray(boxes, np.float64)
        bx1, bx2 = np.clip(b[:, [0, 2]], 0, w).min(), np.clip(b[:, [0, 2]], 0, w).max()
        by1, by2 = np.clip(b[:, [1, 3]], 0, h).min(), np.clip(b[:, [1, 3]], 0, h).max()
        sizes, flips = set(), 0
        for _ in range(2000):
            rec.log.clear()
            crop, jit, flip = D.draw_augment_geom(rec, h, w, boxes, cfg)
            x0, y0, x1, y1 = crop
            assert all(isinstance(v, int) for v in crop) and isinstance(flip, bool), name
            assert jit.dtype == np.float32 and jit.shape == (3,)
            # the documented order: r, ox, oy | cw, ch, x0, y0 | the factors that are on | flip
            kinds = [k for k, _, _ in rec.log]
            assert kinds == ["uniform", "randint", "randint"] + (["uniform", "uniform", "randint", "randint"] + ["uniform"] * 3 if crop_on else ["uniform"]) + ["uniform"], name
            r, ox, oy = rec.log[0][2], int(rec.log[1][2]), int(rec.log[2][2])
            assert 1.0 <= r <= emax
            W, H = max(w, int(round(w * r))), max(h, int(round(h * r)))                    # r, checked through the canvas size
            assert w <= W <= int(round(w * emax)) and h <= H <= int(round(h * emax))
            assert rec.log[1][1] == (0, W - w + 1) and rec.log[2][1] == (0, H - h + 1) and 0 <= ox <= W - w and 0 <= oy <= H - h
            assert 1 <= x1 - x0 <= W and 1 <= y1 - y0 <= H, (name, crop)                   # window sides <= canvas sides
            assert 0 <= x0 + ox and x1 + ox <= W and 0 <= y0 + oy and y1 + oy <= H, (name, crop, (ox, oy, W, H))      # ... and inside the canvas
            assert x0 <= bx1 and bx2 <= x1 and y0 <= by1 and by2 <= y1, (name, crop, boxes)                # holds every clipped box
            if not crop_on:
                assert (x0 + ox, y0 + oy, x1 + ox, y1 + oy) == (0, 0, W, H), "crop off: the window is the whole canvas"
            assert flip == (rec.log[-1][2] < 0.5)
            sizes.add((x1 - x0, y1 - y0))
            flips += flip
        assert len(sizes) > 20 and max(s[0] for s in sizes) > w, "the zoom-out makes windows larger than the image"
        assert 800 < flips < 1200


def test_flip_probability():
    box = [[4, 5, 20, 30]]
    for seed in range(3):
        rng = np.random.RandomState(seed)
        assert all(D.draw_augment_geom(rng, 37, 53, box, config.get_cfg(aug_flip=1.0))[2] is True for _ in range(200)), "aug_flip = 1 always flips"
    rec = Recorder(0)
    for _ in range(200):
        crop, jit, flip = D.draw_augment_geom(rec, 37, 53, box, config.get_cfg(aug_flip=0.0, aug_expand_max=2.0))
        assert flip is False
    assert len(rec.log) == 3 * 200 and [k for k, _, _ in rec.log[:3]] == ["uniform", "randint", "randint"], "aug_flip = 0 draws nothing"
    # flip alone: the whole image, factors 1, one draw
    rec = Recorder(1)
    crop, jit, flip = D.draw_augment_geom(rec, 37, 53, box, config.get_cfg(aug_flip=0.5))
    assert crop == (0, 0, 53, 37) and jit.tolist() == [1.0, 1.0, 1.0] and len(rec.log) == 1
    rng, cfg = np.random.RandomState(11), config.get_cfg(aug_flip=0.5)
    n = sum(D.draw_augment_geom(rng, 37, 53, box, cfg)[2] for _ in range(4000))
    assert abs(n - 2000) <= 4 * np.sqrt(1000), n                                           # 4 standard deviations of Binomial(4000, 0.5)


# ---- 3. boxes and phrases ---------------------------------------------------------------------------------------------------------------------
def test_swap_left_right():
    for text, want in [("the man on the left", "the man on the right"), ("Left person", "Right person"), ("RIGHT", "LEFT"),
                       ("leftmost car", "rightmost car"), ("bright light", "bright light"), ("left_right".replace("_", " "), "right left"),
                       ("a dog in the sky", "a dog in the sky"), ("Righthand side , LEFTMOST", "Lefthand side , RIGHTMOST"),
                       ("leftover rights", "leftover rights"), ("", "")]:
        assert D.swap_left_right(text) == want
        assert D.swap_left_right(D.swap_left_right(text)) == text


@pytest.mark.parametrize("win", [(2, 1, 22, 17), (-3, -2, 18, 15), (1, 2, 39, 29)], ids=["even width", "odd width, overhang", "wide"])
def test_flipped_box_sits_on_the_flipped_pixels(tiny, win):
    g, kw, root = tiny
    ds = D.ImgQuDataset(config.get_cfg(**kw, aug_flip=1.0), root / "d.csv", "refclef", "train")
    row = 3                                                                                # a.png (30 x 40), box [5, 5, 12, 9]
    bx1, by1, bx2, by2 = (int(v) for v in g["csv_bbox"][row])
    img = np.zeros((30, 40, 3), np.uint8)
    img[by1:by2, bx1:bx2] = 255                                                            # the box, painted
    ch, cw = win[3] - win[1], win[2] - win[0]
    ones = np.ones(3, np.float32)
    plain = ds.query_item(row, 30, 40, win)
    it = ds.query_item(row, 30, 40, win, True)
    for flip, item in ((False, plain), (True, it)):
        out = D.augment_host(img, win, ones, (ch, cw), flip=flip, fill=(0, 0, 0))           # output == window: no resampling
        x1, y1, x2, y2 = (int(v) for v in item["orig_annot"].tolist())
        assert (out[y1:y2, x1:x2] == 255).all() and int((out == 255).all(axis=2).sum()) == (y2 - y1) * (x2 - x1) == (by2 - by1) * (bx2 - bx1)
    px1, py1, px2, py2 = plain["orig_annot"].tolist()
    assert it["orig_annot"].tolist() == [cw - px2, py1, cw - px1, py2] and it["img_size"].tolist() == [ch, cw]
    # annot <-> orig_annot <-> img_size: the identity tests/test_cpu_augment.py checks, through the mirror
    back = back_to_image(it["annot"], win)                                                  # x1 y1 x2 y2 of the MIRRORED box, in image pixels
    x0, x1w = win[0], win[2]
    assert np.abs(np.array([x0 + x1w - back[2], back[1], x0 + x1w - back[0], back[3]]) - g["csv_bbox"][row]).max() < 1e-3
    assert np.abs(back_to_image(it["annot"], (0, 0, cw, ch)) - it["orig_annot"].double().numpy()).max() < 1e-4


# ---- 4. the dataset -----------------------------------------------------------------------------------------------------------------------------
def test_dataset_items_with_flip_and_zoom_out(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG, **GEOM)
    raw = {k: g["png_" + k] for k in "abc"}
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)
    ds_h = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train")
    emb = ds_g.embedder
    seen, outside = set(), 0
    for rep in range(6):
        for i in range(5):
            np.random.seed(100 * rep + i)
            it = ds_g[i]
            np.random.seed(100 * rep + i)
            ih = ds_h[i]
            assert set(ih) == ITEM_KEYS and set(it) == ITEM_KEYS | {"aug_crop", "aug_jitter", "aug_geom"}
            crop, jit, geom = it["aug_crop"], it["aug_jitter"], it["aug_geom"]
            assert geom.dtype == torch.int32 and tuple(geom.shape) == (4,) and geom[1:].tolist() == [124, 116, 104] and geom[0].item() in (0, 1)
            flip = bool(geom[0])
            seen.add(flip)
            x0, y0, x1, y1 = crop.tolist()
            im = raw[str(g["csv_img"][i])[0]]
            outside += not (0 <= x0 and 0 <= y0 and x1 <= im.shape[1] and y1 <= im.shape[0])
            assert np.array_equal(it["img"].numpy(), im) and it["img_size"].tolist() == [y1 - y0, x1 - x0]
            for k in ("annot", "orig_annot", "img_size", "qvec", "qlens", "idxs"):
                assert torch.equal(it[k], ih[k]), k
            box = np.asarray(g["csv_bbox"][i], np.float64) - np.array([x0, y0, x0, y0])
            if flip:
                box = np.array([x1 - x0 - box[2], box[1], x1 - x0 - box[0], box[3]])
            assert np.abs(it["orig_annot"].double().numpy() - box).max() < 1e-4
            assert np.abs(back_to_image(it["annot"], (0, 0, x1 - x0, y1 - y0)) - box).max() < 1e-3
            q = str(g["csv_query"][i]).replace("_", " ")
            qvec, qlen = D.embed_query(emb, D.swap_left_right(q) if flip else q)
            assert np.array_equal(it["qvec"].numpy(), qvec) and int(it["qlens"]) == qlen
            want = D.augment_host(im, (x0, y0, x1, y1), jit.numpy(), (40, 48), flip=flip, fill=(124, 116, 104))
            assert torch.equal(ih["img"], torch.from_numpy(want.transpose(2, 0, 1).astype(np.float64)).float().div_(255))
    assert seen == {False, True} and outside > 5
    b = D.collater([ds_g[0], ds_g[2]])
    assert b["aug_geom"].dtype == torch.int32 and tuple(b["aug_geom"].shape) == (2, 4) and b["aug_crop"].dtype == torch.int32
    # row 3's query says "left": flipped, it is embedded as "right" (a word the table does not know: another vector)
    d1 = D.ImgQuDataset(config.get_cfg(**kw, aug_flip=1.0), root / "d.csv", "refclef", "train")
    d0 = D.ImgQuDataset(config.get_cfg(**kw), root / "d.csv", "refclef", "train")
    assert np.array_equal(d1[3]["qvec"].numpy(), D.embed_query(emb, "unknownword right of the tree")[0])
    assert not torch.equal(d1[3]["qvec"], d0[3]["qvec"]) and torch.equal(d1[0]["qvec"], d0[0]["qvec"])
    assert torch.equal(d1[0]["img"], d0[0]["img"].flip(-1)), "flip alone: the plain resize, mirrored"


def test_grouped_training_batch_flips_a_slot_together(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG, **GEOM)
    chunks, rows = [[0, 3], [2, 4]], [0, 3, 2, 4]
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)
    ds_h = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train")
    seen = set()
    for seed in range(8):
        np.random.seed(seed)
        b = ds_g.grouped_train_batch(chunks)
        np.random.seed(seed)
        bh = ds_h.grouped_train_batch(chunks)
        assert b["aug_geom"].dtype == torch.int32 and tuple(b["aug_geom"].shape) == (2, 4) and tuple(b["aug_crop"].shape) == (2, 4)
        assert not any(k.startswith("aug_") for k in bh) and tuple(bh["img"].shape) == (2, 3, 40, 48)
        for k in ("annot", "orig_annot", "img_size", "qvec", "qlens"):
            assert torch.equal(b[k], bh[k]), k
        for q, row in enumerate(rows):
            s = int(b["img_idx"][q])
            x0, y0, x1, y1 = b["aug_crop"][s].tolist()
            flip = bool(b["aug_geom"][s, 0])
            seen.add((s, flip))
            box = np.asarray(g["csv_bbox"][row], np.float64) - np.array([x0, y0, x0, y0])
            if flip:
                box = np.array([x1 - x0 - box[2], box[1], x1 - x0 - box[0], box[3]])
            assert np.abs(b["orig_annot"][q].double().numpy() - box).max() < 1e-4, "every query of a slot is mirrored with the slot"
            text = str(g["csv_query"][row]).replace("_", " ")
            qvec, qlen = D.embed_query(ds_g.embedder, D.swap_left_right(text) if flip else text)
            n = b["qvec"].shape[1]
            assert np.array_equal(b["qvec"][q].numpy(), qvec[:n]) and int(b["qlens"][q]) == qlen
        for s, k in enumerate("ac"):
            want = D.augment_host(g["png_" + k], b["aug_crop"][s].tolist(), b["aug_jitter"][s].numpy(), (40, 48), flip=bool(b["aug_geom"][s, 0]),
                                  fill=b["aug_geom"][s, 1:].tolist())
            assert torch.equal(bh["img"][s], torch.from_numpy(want.transpose(2, 0, 1).astype(np.float64)).float().div_(255))
    assert seen == {(0, False), (0, True), (1, False), (1, True)}
    assert not any(k.startswith("aug_") for k in ds_g.grouped_batch([0, 3, 2]))            # the grouped VALIDATION batch is never augmented


def test_validation_is_the_golden_and_old_configurations_keep_their_fields(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG, **GEOM)
    data = D.get_data(cfg, prefetch=False)
    assert data.train_dl.dataset.augment and not data.valid_dl.dataset.augment and not data.test_dl["test0"].dataset.augment
    np.random.seed(0)
    tr = list(data.train_dl)
    assert len(tr) == 1 and not any(k.startswith("aug_") for k in tr[0])
    dv = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "valid")
    for i in range(5):
        it = dv[i]
        assert set(it) == ITEM_KEYS
        for k, v in it.items():
            assert np.array_equal(v.numpy(), g[f"item{i}_{k}"]), (i, k)
    # the new keys off: items and batches carry exactly the fields they carried before
    d_old = D.ImgQuDataset(config.get_cfg(**kw, **AUG), root / "d.csv", "refclef", "train", gpu_resize=True)
    assert d_old.aug_fill is None and set(d_old[0]) == ITEM_KEYS | {"aug_crop", "aug_jitter"}
    assert set(d_old.grouped_train_batch([[0, 3], [2, 4]])) == ITEM_KEYS | {"aug_crop", "aug_jitter", "img_idx", "img_hw"}
    d_off = D.ImgQuDataset(config.get_cfg(**kw), root / "d.csv", "refclef", "train", gpu_resize=True)
    assert not d_off.augment and set(d_off[0]) == ITEM_KEYS
    # ... and a seeded item of an old configuration is what draw_augment gives
    np.random.seed(5)
    it = d_old[2]
    np.random.seed(5)
    crop, jit = D.draw_augment(np.random, 64, 64, [g["csv_bbox"][2].tolist()], config.get_cfg(**AUG))
    assert it["aug_crop"].tolist() == list(crop) and np.array_equal(it["aug_jitter"].numpy(), jit)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------------
def test_interface_and_errors(tiny, gold):
    g, kw, root = tiny
    from zsgnet_pytorch_amd import _lib as L
    assert "zsg_augment_geom_u8_batched" in open(os.path.join(ROOT, "include", "zsg.h")).read()
    assert "zsg_augment_geom_u8_batched" in L.SIGNATURES and hasattr(L.lib, "zsg_augment_geom_u8_batched")
    assert len(L.SIGNATURES["zsg_augment_geom_u8_batched"][1]) == 10
    assert config.get_cfg()["aug_flip"] == 0.0 and config.get_cfg()["aug_expand_max"] == 1.0 and config.get_cfg()["aug_fill"] == [124, 116, 104]
    for key, bad in (("aug_flip", dict(aug_flip=-0.1)), ("aug_flip", dict(aug_flip=1.01)), ("aug_flip", dict(aug_flip=float("nan"))),
                     ("aug_expand_max", dict(aug_expand_max=0.99)), ("aug_expand_max", dict(aug_expand_max=4.5)),
                     ("aug_expand_max", dict(aug_expand_max=float("inf"))), ("aug_fill", dict(aug_fill=[1, 2])), ("aug_fill", dict(aug_fill=[1, 2, 256])),
                     ("aug_fill", dict(aug_fill=[-1, 2, 3])), ("aug_fill", dict(aug_fill=[1.5, 2, 3])), ("aug_fill", dict(aug_fill=[1, 2, 3, 4]))):
        with pytest.raises(ValueError, match=key):
            D.get_data(config.get_cfg(**kw, **bad), prefetch=False)
    D.get_data(config.get_cfg(**kw, aug_flip=1.0, aug_expand_max=4.0, aug_fill=[0, 255, 3]), prefetch=False)      # the ends of the ranges are valid
    from zsgnet_pytorch_amd.main_dist import learner_init
    for on in (dict(aug_flip=0.5), dict(aug_expand_max=2.0)):
        with pytest.raises(ValueError, match="synthetic"):
            learner_init("x", config.get_cfg(synthetic=True, **on))
    a, ones = images(gold)[3], np.ones(3, np.float32)
    for bad in [(-1, 0, 5, 5), (0, 0, 54, 5), (5, 5, 5, 9), (0, 30, 5, 38)]:
        with pytest.raises(ValueError, match="is not inside"):
            D.augment_host(a, bad, ones, (24, 32))
        with pytest.raises(ValueError, match="is not inside"):
            D.augment_host(a, bad, ones, (24, 32), flip=True)
    for empty in [(5, 5, 5, 9), (7, 3, 2, 9), (0, 4, 9, 4)]:
        with pytest.raises(ValueError, match="crop"):
            D.augment_host(a, empty, ones, (24, 32), fill=FILL)
    for bad_fill in [(1, 2), (1, 2, 300), (0.5, 1, 2), "abc"]:
        with pytest.raises(ValueError, match="fill"):
            D.augment_host(a, (-1, 0, 5, 5), ones, (24, 32), fill=bad_fill)

"""Training augmentation on the host: dat_loader.draw_augment (box-safe random crop + jitter factors), dat_loader.augment_host (THE
byte-exact definition the HIP kernels of csrc/aug.hip reproduce: tests/test_gpu_augment.py) against Pillow and against the independent
restatement tests/augment_ref.py, and the loader plumbing (items, grouped training batches, cfg validation)."""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from zsgnet_pytorch_amd import config, dat_loader as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = dict(aug_crop_min=0.3, aug_brightness=0.3, aug_contrast=0.4, aug_saturation=1.5)
TRIPLES = [(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2), (0.7, 1.3, 0.6)]
OUTS = [(24, 32), (40, 48)]                      # (Ho, Wo)


def images(gold):
    g = gold("g13_dataset")
    return [np.ascontiguousarray(g["png_" + k]) for k in "abc"] + [np.random.RandomState(7).randint(0, 256, (37, 53, 3)).astype(np.uint8)]


def windows(h, w):
    """whole image, 1 pixel high, 1 pixel wide, touching the right and bottom borders, smaller than either output (upscales)"""
    return [(0, 0, w, h), (0, h // 2, w, h // 2 + 1), (w // 3, 0, w // 3 + 1, h), (w - 11, h - 9, w, h), (2, 3, 15, 13)]


# ---- draw_augment -------------------------------------------------------------------------------------------------------------------
def box_cases(h, w):
    return {"corner": [[w - 6.0, h - 5.0, w, h]], "corner0": [[0, 0, 5, 4]], "larger than the window": [[2, 3, w - 2, h - 3]],
            "whole image": [[0, 0, w, h]], "zero area": [[10, 12, 10, 12]], "partly outside": [[-5.5, 20, 30.25, h + 10]],
            "three boxes": [[4, 5, 9.5, 11], [20.5, 3, 31, 8], [7, 25, 12, 30.75]]}


@pytest.mark.parametrize("hw", [(37, 53), (64, 48)])
def test_draw_augment_invariants(hw):
    h, w = hw
    cfg = config.get_cfg(**AUG)
    f32 = np.float32
    lo = [f32(0.7), f32(0.6), f32(0.0)]
    hi = [f32(1.3), f32(1.4), f32(2.5)]
    for name, boxes in box_cases(h, w).items():
        rng = np.random.RandomState(11)
        b = np.asarray(boxes, np.float64)
        bx1, bx2 = np.clip(b[:, [0, 2]], 0, w).min(), np.clip(b[:, [0, 2]], 0, w).max()
        by1, by2 = np.clip(b[:, [1, 3]], 0, h).min(), np.clip(b[:, [1, 3]], 0, h).max()
        widths = set()
        for _ in range(2000):
            crop, jit = D.draw_augment(rng, h, w, boxes, cfg)
            x0, y0, x1, y1 = crop
            assert all(isinstance(v, int) for v in crop), name
            assert 0 <= x0 and 0 <= y0 and x1 <= w and y1 <= h and x1 - x0 >= 1 and y1 - y0 >= 1, (name, crop)
            assert x0 <= bx1 and bx2 <= x1 and y0 <= by1 and by2 <= y1, (name, crop, boxes)       # holds every clipped box
            assert jit.dtype == np.float32 and jit.shape == (3,)
            assert all(lo[i] <= jit[i] <= hi[i] for i in range(3)), (name, jit)
            widths.add(x1 - x0)
        if name == "whole image":
            assert widths == {w}
        elif name == "larger than the window":
            assert min(widths) == w - 4, "a drawn window smaller than the box is enlarged to exactly the box"
        else:
            assert len(widths) > 5, "the window size varies"
            if name in ("corner", "corner0", "zero area"):
                assert min(widths) < 0.5 * w, "small boxes leave room for small windows"


def test_draw_augment_defaults_and_single_parts():
    rng = np.random.RandomState(0)
    assert D.draw_augment(rng, 37, 53, [[1, 2, 3, 4]], config.get_cfg()) is None
    assert D.draw_augment(rng, 37, 53, [[1, 2, 3, 4]], {}) is None                         # a cfg without the keys = the defaults
    crop, jit = D.draw_augment(rng, 37, 53, [[1, 2, 3, 4]], config.get_cfg(aug_contrast=0.5))
    assert crop == (0, 0, 53, 37) and jit[0] == 1.0 and jit[2] == 1.0 and 0.5 <= jit[1] <= 1.5      # crop off: the whole image
    crop, jit = D.draw_augment(rng, 37, 53, [[1, 2, 3, 4]], config.get_cfg(aug_crop_min=0.5))
    assert jit.tolist() == [1.0, 1.0, 1.0] and crop[2] - crop[0] >= 26                     # a key at 0: the factor is exactly 1
    # the same seed gives the same draw
    a = D.draw_augment(np.random.RandomState(3), 64, 48, [[5, 5, 9, 9]], config.get_cfg(**AUG))
    b = D.draw_augment(np.random.RandomState(3), 64, 48, [[5, 5, 9, 9]], config.get_cfg(**AUG))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ---- augment_host ---------------------------------------------------------------------------------------------------------------------
def test_augment_host_step1_is_pillow_crop_resize(gold):
    import PIL.Image
    ones = np.ones(3, np.float32)
    for a in images(gold):
        h, w = a.shape[:2]
        for (Ho, Wo) in OUTS:
            for win in windows(h, w):
                ref = np.asarray(PIL.Image.fromarray(a).crop(win).resize((Wo, Ho)))
                got = D.augment_host(a, win, ones, (Ho, Wo))
                assert got.dtype == np.uint8 and got.shape == (Ho, Wo, 3)
                assert np.array_equal(got, ref), f"{(h, w)} window {win} -> {(Ho, Wo)}: differs from Pillow's crop().resize()"
            today = np.asarray(PIL.Image.fromarray(a).resize((Wo, Ho)))                  # the loader's path without augmentation
            assert np.array_equal(D.augment_host(a, (0, 0, w, h), ones, (Ho, Wo)), today)
    for bad in [(-1, 0, 5, 5), (0, 0, 54, 5), (5, 5, 5, 9), (0, 30, 5, 38)]:
        with pytest.raises(ValueError, match="crop"):
            D.augment_host(images(gold)[3], bad, ones, (24, 32))


def test_augment_host_equals_the_independent_restatement(gold):
    for n, a in enumerate(images(gold)):
        h, w = a.shape[:2]
        win = windows(h, w)[3] if n % 2 else (1, 2, w - 3, h - 1)
        for t in TRIPLES:
            got = D.augment_host(a, win, np.array(t, np.float32), OUTS[0])
            assert np.array_equal(got, R.augment(a, win, t, OUTS[0])), f"image {n} window {win} factors {t}"
    a = images(gold)[3]
    assert np.array_equal(D.augment_host(a, (0, 0, 53, 37), np.array(TRIPLES[-1], np.float32), OUTS[1]), R.augment(a, (0, 0, 53, 37), TRIPLES[-1], OUTS[1]))


def test_augment_host_hand_checked_facts(gold):
    a = images(gold)[2]                            # 64 x 64
    win, out = (3, 5, 60, 50), (24, 32)
    f = lambda *t: D.augment_host(a, win, np.array(t, np.float32), out)
    base = R.step1(a, win, out)
    assert np.array_equal(f(1, 1, 1), base)                                               # all-ones factors: the resized crop itself
    assert not f(0, 1, 1).any()                                                           # brightness 0: black
    c0 = f(1, 0, 1)
    grays = [R.gray(*base[y, x]) for y in range(24) for x in range(32)]
    mean = np.float32(np.float64(sum(grays)) / np.float64(24 * 32))
    assert (c0 == int(mean)).all() and 0 < int(mean) < 255                                # contrast 0: the constant trunc(mean)
    s0 = f(1, 1, 0)
    assert np.array_equal(s0[..., 0], s0[..., 1]) and np.array_equal(s0[..., 1], s0[..., 2])
    assert np.array_equal(s0[..., 0].reshape(-1), np.array(grays, np.uint8))              # saturation 0: r == g == b == gray
    b2 = f(2, 1, 1)
    assert np.array_equal(b2, np.minimum(2 * base.astype(np.int32), 255).astype(np.uint8)) and (b2 == 255).any()      # factor 2 clamps


# ---- the loader -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tiny(tmp_path, gold):
    import PIL.Image
    g = gold("g13_dataset")
    for k in "abc":
        PIL.Image.fromarray(g["png_" + k]).save(tmp_path / f"{k}.png")
    with open(tmp_path / "d.csv", "w") as f:
        f.write("img_id,bbox,query\n")
        for i, b, q in zip(g["csv_img"], g["csv_bbox"], g["csv_query"]):
            f.write(f'{i},"{[float(v) for v in b]}","{q}"\n')
    np.savez(tmp_path / "vec.npz", words=g["words"], vectors=g["table"])
    kw = dict(resize_img=[int(v) for v in g["resize_img"]], word_vectors=str(tmp_path / "vec.npz"), ds_to_use="refclef", bs=3, bsv=2, nw=0, nwv=0,
              **{"ds_info.refclef.img_dir": str(tmp_path), "ds_info.refclef.trn_csv_file": str(tmp_path / "d.csv"),
                 "ds_info.refclef.val_csv_file": str(tmp_path / "d.csv"), "ds_info.refclef.test_csv_file": str(tmp_path / "d.csv")})
    return g, kw, tmp_path


def back_to_image(annot, crop):
    """(annot + 1) / 2 * (ch, cw, ch, cw) + (y0, x0, y0, x0) -> the box in the decoded image, as x1 y1 x2 y2"""
    x0, y0, x1, y1 = (float(v) for v in crop)
    ch, cw = y1 - y0, x1 - x0
    y1x1y2x2 = (annot.double().numpy() + 1) / 2 * np.array([ch, cw, ch, cw]) + np.array([y0, x0, y0, x0])
    return y1x1y2x2[[1, 0, 3, 2]]


def test_dataset_items_with_augmentation(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG)
    raw = {k: g["png_" + k] for k in "abc"}
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)        # the raw image travels, the GPU augments
    ds_h = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train")                         # the worker augments (augment_host)
    assert ds_g.augment and ds_h.augment
    for rep in range(4):
        for i in range(5):
            np.random.seed(100 * rep + i)
            it = ds_g[i]
            np.random.seed(100 * rep + i)
            ih = ds_h[i]
            assert set(it) == set(ih) | {"aug_crop", "aug_jitter"} and "aug_crop" not in ih
            crop, jit = it["aug_crop"], it["aug_jitter"]
            assert crop.dtype == torch.int32 and tuple(crop.shape) == (4,) and jit.dtype == torch.float32 and tuple(jit.shape) == (3,)
            x0, y0, x1, y1 = crop.tolist()
            im = raw[str(g["csv_img"][i])[0]]
            assert it["img"].dtype == torch.uint8 and np.array_equal(it["img"].numpy(), im)            # raw, as today
            assert it["img_size"].tolist() == [y1 - y0, x1 - x0]
            box = np.asarray(g["csv_bbox"][i], np.float64)
            assert np.abs(back_to_image(it["annot"], crop) - box).max() < 1e-3
            assert np.abs(it["orig_annot"].double().numpy() - (box - np.array([x0, y0, x0, y0]))).max() < 1e-4
            # the host path drew the same augmentation and applied it: final size, float CHW
            for k in ("annot", "orig_annot", "img_size", "qvec", "qlens", "idxs"):
                assert torch.equal(it[k], ih[k]), k
            want = D.augment_host(im, (x0, y0, x1, y1), jit.numpy(), (40, 48))
            assert tuple(ih["img"].shape) == (3, 40, 48)
            assert torch.equal(ih["img"], torch.from_numpy(want.transpose(2, 0, 1).astype(np.float64)).float().div_(255))
    b = D.collater([ds_g[0], ds_g[2]])
    assert b["aug_crop"].dtype == torch.int32 and tuple(b["aug_crop"].shape) == (2, 4)                 # not cast to float
    assert b["aug_jitter"].dtype == torch.float32 and tuple(b["aug_jitter"].shape) == (2, 3) and "img_hw" in b


def test_get_data_trains_augmented_and_validates_unchanged(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG)
    data = D.get_data(cfg, prefetch=False)
    assert data.train_dl.dataset.augment and not data.valid_dl.dataset.augment and not data.test_dl["test0"].dataset.augment
    np.random.seed(0)
    tr = list(data.train_dl)
    assert len(tr) == 1
    assert tuple(tr[0]["img"].shape) in ((3, 3, 40, 48), (3, 40, 48, 3))                  # resize_img = [W, H] = [48, 40]
    assert not any(k.startswith("aug_") for k in tr[0])
    # validation / test items are the reference's, bit for bit (tests/golden/g13_dataset.npz)
    dv = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "valid")
    for i in range(5):
        it = dv[i]
        assert set(it) == {"img", "idxs", "qvec", "qlens", "annot", "orig_annot", "img_size"}
        for k, v in it.items():
            assert np.array_equal(v.numpy(), g[f"item{i}_{k}"]), (i, k)
    # defaults: a training item carries no aug_* field and is today's item
    d0 = D.ImgQuDataset(config.get_cfg(**kw), root / "d.csv", "refclef", "train", gpu_resize=True)
    assert not d0.augment and set(d0[0]) == {"img", "idxs", "qvec", "qlens", "annot", "orig_annot", "img_size"}
    d1 = D.ImgQuDataset(config.get_cfg(**kw), root / "d.csv", "refclef", "train")
    assert all(np.array_equal(v.numpy(), g[f"item1_{k}"]) for k, v in d1[1].items())


def test_grouped_training_batches_share_one_crop_per_slot(tiny):
    g, kw, root = tiny
    cfg = config.get_cfg(**kw, **AUG)
    chunks = [[0, 3], [2, 4]]                      # rows 0, 3 share a.png; rows 2, 4 share c.png
    ds_g = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train", gpu_resize=True)
    ds_h = D.ImgQuDataset(cfg, root / "d.csv", "refclef", "train")
    for seed in range(6):
        np.random.seed(seed)
        b = ds_g.grouped_train_batch(chunks)
        np.random.seed(seed)
        bh = ds_h.grouped_train_batch(chunks)
        assert b["aug_crop"].dtype == torch.int32 and tuple(b["aug_crop"].shape) == (2, 4)
        assert b["aug_jitter"].dtype == torch.float32 and tuple(b["aug_jitter"].shape) == (2, 3)
        assert b["img_idx"].tolist() == [0, 0, 1, 1] and b["img_hw"].tolist() == [[30, 40], [64, 64]]
        for q, row in enumerate([0, 3, 2, 4]):
            crop = b["aug_crop"][b["img_idx"][q]]
            x0, y0, x1, y1 = crop.tolist()
            box = np.asarray(g["csv_bbox"][row], np.float64)
            assert x0 <= box[0] and box[2] <= x1 and y0 <= box[1] and box[3] <= y1, "the slot's crop holds every box of its chunk"
            assert np.abs(back_to_image(b["annot"][q], crop) - box).max() < 1e-3            # every query uses its slot's crop
            assert b["img_size"][q].tolist() == [y1 - y0, x1 - x0]
        assert not any(k.startswith("aug_") for k in bh) and tuple(bh["img"].shape) == (2, 3, 40, 48)
        assert torch.equal(bh["annot"], b["annot"]) and torch.equal(bh["img_size"], b["img_size"])
        for s, k in enumerate("ac"):
            want = D.augment_host(g["png_" + k], b["aug_crop"][s].tolist(), b["aug_jitter"][s].numpy(), (40, 48))
            assert torch.equal(bh["img"][s], torch.from_numpy(want.transpose(2, 0, 1).astype(np.float64)).float().div_(255))
    # the grouped VALIDATION batch is never augmented
    bv = ds_g.grouped_batch([0, 3, 2])
    assert not any(k.startswith("aug_") for k in bv)


def test_interface_and_errors(tiny):
    g, kw, root = tiny
    from zsgnet_pytorch_amd import _lib as L
    assert "zsg_augment_u8_batched" in open(os.path.join(ROOT, "include", "zsg.h")).read()
    assert "zsg_augment_u8_batched" in L.SIGNATURES and hasattr(L.lib, "zsg_augment_u8_batched")
    assert len(L.SIGNATURES["zsg_augment_u8_batched"][1]) == 9
    for bad in (dict(aug_crop_min=0.0), dict(aug_crop_min=1.5), dict(aug_crop_min=-0.2), dict(aug_brightness=-0.1),
                dict(aug_contrast=-1.0), dict(aug_saturation=-0.5), dict(aug_contrast=float("inf"))):
        with pytest.raises(ValueError, match="aug_"):
            D.get_data(config.get_cfg(**kw, **bad), prefetch=False)
    from zsgnet_pytorch_amd.main_dist import learner_init
    with pytest.raises(ValueError, match="synthetic"):
        learner_init("x", config.get_cfg(synthetic=True, aug_brightness=0.2))
    with pytest.raises(ValueError, match="synthetic"):
        learner_init("x", config.get_cfg(synthetic=True, aug_crop_min=0.5))

"""Zoom-out and horizontal flip of the training augmentation on the GPU: zsg_augment_geom_u8_batched (csrc/aug.hip) through
GpuResizer.resize_flat(..., crop, jitter, flip, fill) against the byte-exact host definition dat_loader.augment_host(..., flip, fill)
(itself pinned to Pillow by tests/test_cpu_augment_geom.py) — byte equality everywhere, no tolerance — then the loader end to end."""
import struct

import numpy as np
import pytest
import torch

from zsgnet_pytorch_amd import config, dat_loader as D

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 48), (30, 40)]             # (h, w): 5883 and 9216 bytes, so the second and third image start off a dword boundary
TRIPLES = [(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2), (0.7, 1.3, 0.6)]
OUTS = [(24, 32), (40, 48), (25, 31)]              # (Ho, Wo): whole blocks | a partial last block | odd width, 93-byte rows, a byte tail
FILL = (124, 116, 104)
SENTINEL = 0xA5


def windows(h, w, out_hw):
    """whole image | inside | overhang left + top | right + bottom | all four sides | 3x the image, off-centre | one image pixel in the
    window's corner (top-left, bottom-right) | window == output with overhang (identity tables) | width == output width | beside the
    image, touching nothing | above it"""
    Ho, Wo = out_hw
    return [(0, 0, w, h), (2, 3, 15, 13), (-5, -4, w - 3, h - 2), (4, 3, w + 7, h + 6), (-3, -2, w + 5, h + 4),
            (-w - 5, -(h // 2), 2 * w - 5, 3 * h - h // 2), (w - 1, h - 1, w + 19, h + 16), (-18, -21, 1, 1), (-3, -2, Wo - 3, Ho - 2),
            (w - 9, 1, w - 9 + Wo, h - 1), (w + 3, 2, w + 20, 15), (1, -30, 20, -5)]


@pytest.fixture(scope="module")
def batch():
    """36 jobs: every window kind on each of the three images; the flat buffer holds the three images twelve times over"""
    rng = np.random.RandomState(5)
    three = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    imgs = three * 12
    flat, hw = D.flatten_raw([torch.from_numpy(a) for a in imgs])
    return imgs, flat.cuda(), hw


def jobs_for(out_hw, rot=0):
    crops = [windows(*SIZES[i % 3], out_hw)[i // 3] for i in range(36)]
    flips = [bool((i + i // 3 + rot) % 2) for i in range(36)]                              # each window kind flipped and not, on different images
    jit = np.array([TRIPLES[(i + rot) % 8] for i in range(36)], np.float32)
    fills = np.array([FILL if i % 5 else (0, 255, 7) for i in range(36)], np.int32)
    return crops, jit, flips, fills


_REF = {}


def host(imgs, crops, jit, flips, fills, out_hw):
    """augment_host of every job, computed once per (jobs, output size) and kept read-only"""
    key = (tuple(map(tuple, crops)), np.asarray(jit, np.float32).tobytes(), tuple(flips), np.asarray(fills).tobytes(), tuple(out_hw), len(imgs))
    if key not in _REF:
        ref = np.stack([D.augment_host(a, c, np.asarray(j, np.float32), out_hw, flip=bool(f), fill=tuple(int(v) for v in fl))
                        for a, c, j, f, fl in zip(imgs, crops, jit, flips, fills)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def assert_jobs_equal(got, ref, crops, jit, flips, out_hw):
    got = got.cpu().numpy()
    for i in range(len(crops)):
        assert np.array_equal(got[i], ref[i]), f"job {i}: {SIZES[i % 3]} window {crops[i]} flip {flips[i]} factors {jit[i].tolist()} -> {out_hw}"


@pytest.mark.parametrize("out_hw", OUTS)
def test_resize_flat_with_crop_jitter_flip_fill_is_augment_host(batch, out_hw):
    imgs, flat, hw = batch
    rz = D.GpuResizer(out_hw)
    for rot in (0, 3):                             # between the two batches every window kind meets both flips and other factors
        crops, jit, flips, fills = jobs_for(out_hw, rot)
        got = rz.resize_flat(flat, hw, crop=torch.tensor(crops, dtype=torch.int32), jitter=torch.from_numpy(jit), flip=torch.tensor(flips),
                             fill=torch.from_numpy(fills))
        torch.cuda.synchronize()
        assert_jobs_equal(got, host(imgs, crops, jit, flips, fills, out_hw), crops, jit, flips, out_hw)
    assert rz.launches == {"augment_u8": 0, "augment_geom_u8": 2}
    # one fill colour for the whole batch; a flip without fill (inside windows only)
    crops, jit, flips, _ = jobs_for(out_hw)
    got = rz.resize_flat(flat, hw, crop=crops, jitter=jit, fill=FILL)
    inside = [windows(*SIZES[i % 3], out_hw)[i % 2] for i in range(36)]
    flipped = rz.resize_flat(flat, hw, crop=inside, flip=flips)
    torch.cuda.synchronize()
    assert_jobs_equal(got, host(imgs, crops, jit, [False] * 36, [FILL] * 36, out_hw), crops, jit, [False] * 36, out_hw)
    assert_jobs_equal(flipped, host(imgs, inside, np.ones((36, 3), np.float32), flips, [FILL] * 36, out_hw), inside, np.ones((36, 3)), flips, out_hw)
    # without fill a window that leaves its image is still refused, with or without flips; an empty window always
    for bad in ((0, 0, 54, 37), (-1, 0, 5, 5), (5, 5, 5, 9), (0, 30, 5, 38)):
        with pytest.raises(ValueError, match="is not inside"):
            rz.resize_flat(flat, hw, crop=[bad] + inside[1:], flip=flips)
        with pytest.raises(ValueError, match="is not inside"):
            rz.resize_flat(flat, hw, crop=[bad] + inside[1:])
    for bad in ((5, 5, 5, 9), (9, 2, 3, 8)):
        with pytest.raises(ValueError, match="crop"):
            rz.resize_flat(flat, hw, crop=[bad] + inside[1:], fill=FILL)
    with pytest.raises(ValueError, match="fill"):
        rz.resize_flat(flat, hw, crop=inside, fill=(1, 2, 256))
    with pytest.raises(ValueError, match="flips"):
        rz.resize_flat(flat, hw, crop=inside, flip=[True] * 35)
    with pytest.raises(ValueError, match="sides"):
        rz.resize_flat(flat, hw, crop=[(-40000, 0, 5, 5)] + inside[1:], fill=FILL)


@pytest.mark.parametrize("out_hw", OUTS)
def test_old_and_new_entry_agree_and_old_batches_keep_the_old_kernels(batch, out_hw):
    imgs, flat, hw = batch
    rz = D.GpuResizer(out_hw)
    inside = [windows(*SIZES[i % 3], out_hw)[i % 2] for i in range(36)]
    jit = np.array([TRIPLES[i % 8] for i in range(36)], np.float32)
    old = rz.resize_flat(flat, hw, crop=inside, jitter=jit).clone()
    assert rz.launches == {"augment_u8": 1, "augment_geom_u8": 0}
    with_fill = rz.resize_flat(flat, hw, crop=inside, jitter=jit, flip=[False] * 36, fill=FILL).clone()
    assert rz.launches == {"augment_u8": 2, "augment_geom_u8": 0}, "no flipped job and no window outside its image: today's kernels"
    items = [(flat.data_ptr() + off, h, w, *c) for (off, h, w), c in zip(rz._offsets(hw), inside)]
    new = rz._run_aug_geom(items, jit, [False] * 36, [FILL] * 36, None)                    # the same jobs through the new entry
    torch.cuda.synchronize()
    assert rz.launches == {"augment_u8": 2, "augment_geom_u8": 1}
    assert torch.equal(old, new) and torch.equal(old, with_fill)
    assert np.array_equal(old.cpu().numpy(), host(imgs, inside, jit, [False] * 36, [FILL] * 36, out_hw))
    one_flip = rz.resize_flat(flat, hw, crop=inside, jitter=jit, flip=[False] * 35 + [True])
    torch.cuda.synchronize()
    assert rz.launches == {"augment_u8": 2, "augment_geom_u8": 2}, "one flipped job sends the batch through the new entry"
    assert torch.equal(one_flip[:35], old[:35]) and torch.equal(one_flip[35], old[35].flip(1))


def test_repeat_run_accumulators_and_skipped_third_launch(batch):
    imgs, flat, hw = batch
    out_hw = OUTS[2]
    rz = D.GpuResizer(out_hw)
    crops, jit, flips, fills = jobs_for(out_hw, 1)
    ref = host(imgs, crops, jit, flips, fills, out_hw)
    gray = [int(D.augment_host(a, c, np.array([j[0], 1, 0], np.float32), out_hw, fill=tuple(int(v) for v in fl))[..., 0].astype(np.int64).sum())
            for a, c, j, fl in zip(imgs, crops, jit, fills)]                               # sum of gray after brightness (the flip does not move it)
    first = rz.resize_flat(flat, hw, crop=crops, jitter=jit, flip=flips, fill=fills).clone()
    again = rz.resize_flat(flat, hw, crop=crops, jitter=jit, flip=flips, fill=fills)
    torch.cuda.synchronize()
    assert torch.equal(first, again)
    assert_jobs_equal(again, ref, crops, jit, flips, out_hw)
    assert rz._gray[:36].tolist() == gray, "the accumulators are zeroed by every call, not added to"
    only_b = np.ones((36, 3), np.float32)
    only_b[:, 0] = [(1, 0, 2, 0.7, 1.3, 0.5)[i % 6] for i in range(36)]                    # contrast = saturation = 1 everywhere: launch 3 is skipped
    got = rz.resize_flat(flat, hw, crop=crops, jitter=only_b, flip=flips, fill=fills)
    torch.cuda.synchronize()
    assert_jobs_equal(got, host(imgs, crops, only_b, flips, fills, out_hw), crops, only_b, flips, out_hw)


@pytest.mark.parametrize("out_hw", OUTS)
def test_nothing_outside_the_output_is_written(batch, out_hw):
    imgs, flat, hw = batch
    rz = D.GpuResizer(out_hw)
    crops, jit, flips, fills = jobs_for(out_hw, 2)
    buf = torch.full((38, out_hw[0], out_hw[1], 3), SENTINEL, dtype=torch.uint8, device="cuda")      # one image of sentinels in front and behind
    got = rz.resize_flat(flat, hw, out=buf[1:37], crop=crops, jitter=jit, flip=flips, fill=fills)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[1].data_ptr()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[37] == SENTINEL).all()), "a store left [B, Ho, Wo, 3]"
    assert_jobs_equal(buf[1:37], host(imgs, crops, jit, flips, fills, out_hw), crops, jit, flips, out_hw)


def test_photo_size_batch_from_the_draw():
    rng = np.random.RandomState(9)
    cfg = config.get_cfg(aug_crop_min=0.4, aug_brightness=0.4, aug_contrast=0.4, aug_saturation=0.7, aug_flip=0.5, aug_expand_max=3.0)
    imgs, crops, jit, flips = [], [], [], []
    for i in range(6):
        h, w = (375, 500) if i % 3 else (500, 333)
        imgs.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        x1, y1 = rng.uniform(0, w - 40), rng.uniform(0, h - 40)
        c, j, f = D.draw_augment_geom(rng, h, w, [[x1, y1, x1 + rng.uniform(5, 40), y1 + rng.uniform(5, 40)]], cfg)
        crops.append(c)
        jit.append(j)
        flips.append(f)
    assert any(flips) and not all(flips) and any(c[0] < 0 or c[2] > a.shape[1] for c, a in zip(crops, imgs))
    flat, hw = D.flatten_raw([torch.from_numpy(a) for a in imgs])
    got = D.GpuResizer((300, 300)).resize_flat(flat.cuda(), hw, crop=crops, jitter=np.stack(jit), flip=flips, fill=FILL)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for i in range(6):
        assert np.array_equal(got[i], D.augment_host(imgs[i], crops[i], jit[i], (300, 300), flip=flips[i], fill=FILL)), \
            f"image {i}: {imgs[i].shape} window {crops[i]} flip {flips[i]} factors {jit[i]}"


def test_loader_end_to_end(tmp_path, gold):
    import PIL.Image
    g = gold("g13_dataset")
    for k in "abc":
        PIL.Image.fromarray(g["png_" + k]).save(tmp_path / f"{k}.png")
    with open(tmp_path / "d.csv", "w") as f:
        f.write("img_id,bbox,query\n")
        for i, b, q in zip(g["csv_img"], g["csv_bbox"], g["csv_query"]):
            f.write(f'{i},"{[float(v) for v in b]}","{q}"\n')
    np.savez(tmp_path / "vec.npz", words=g["words"], vectors=g["table"])
    kw = {"resize_img": [96, 64], "word_vectors": str(tmp_path / "vec.npz"), "ds_to_use": "refclef", "bs": 2, "bsv": 2, "nw": 0, "nwv": 0,
          "resnet_arch": "resnet18", "synthetic": False, "tmp_path": str(tmp_path / "run"),
          "aug_crop_min": 0.4, "aug_brightness": 0.4, "aug_contrast": 0.4, "aug_saturation": 0.5,
          "aug_flip": 0.5, "aug_expand_max": 2.5, "aug_fill": [10, 200, 30],
          "ds_info.refclef.img_dir": str(tmp_path), "ds_info.refclef.trn_csv_file": str(tmp_path / "d.csv"),
          "ds_info.refclef.val_csv_file": str(tmp_path / "d.csv"), "ds_info.refclef.test_csv_file": str(tmp_path / "d.csv")}
    cfg = config.get_cfg(**kw)
    raw = {str(n): g["png_" + str(n)[0]] for n in g["csv_img"]}

    def one_pass(prefetch):
        data = D.get_data(cfg, prefetch=prefetch)
        torch.manual_seed(3)                       # the training loader's shuffle
        np.random.seed(3)                          # the augmentation draws
        return data, [{k: v.cpu() for k, v in b.items()} for b in data.train_dl]

    dg, gpu_batches = one_pass(True)               # raw images + aug_crop / aug_jitter / aug_geom -> DevicePrefetcher -> the GPU
    dh, host_batches = one_pass(False)             # augment_host in the (in-process) worker
    torch.cuda.synchronize()
    assert isinstance(dg.train_dl, D.DevicePrefetcher) and dg.train_dl.loader.dataset.gpu_resize and not dh.train_dl.dataset.gpu_resize
    assert len(gpu_batches) == len(host_batches) == 2
    for bg, bh in zip(gpu_batches, host_batches):
        assert not any(k.startswith("aug_") for k in bg) and "img_hw" not in bg
        assert set(bg) == set(bh)
        assert bg["img"].dtype == torch.uint8 and tuple(bg["img"].shape) == (2, 64, 96, 3)
        for k in ("img", "annot", "orig_annot", "img_size", "idxs", "qlens", "qvec"):
            assert torch.equal(bg[k], bh[k]), k
    # ... and each delivered image is augment_host of the draw, recomputed from the same seed with the dataset alone
    ds = dg.train_dl.loader.dataset
    np.random.seed(3)
    order = [int(i) for b in gpu_batches for i in b["idxs"]]                               # (nw = 0: the items were drawn in this order)
    for pos, i in enumerate(order):
        it = ds[i]
        flip, fill = bool(it["aug_geom"][0]), tuple(it["aug_geom"][1:].tolist())
        assert fill == (10, 200, 30)
        want = D.augment_host(raw[str(g["csv_img"][i])], it["aug_crop"].tolist(), it["aug_jitter"].numpy(), (64, 96), flip=flip, fill=fill)
        assert np.array_equal(gpu_batches[pos // 2]["img"][pos % 2].numpy(), want), (pos, i)
        assert torch.equal(gpu_batches[pos // 2]["orig_annot"][pos % 2], it["orig_annot"])
    launches = dg.train_dl._resizer.launches
    assert launches["augment_u8"] + launches["augment_geom_u8"] == 2 and launches["augment_geom_u8"] >= 1
    # validation batches are never augmented: the same on either path
    vg, vh = next(iter(dg.valid_dl)), next(iter(dh.valid_dl))
    torch.cuda.synchronize()
    assert torch.equal(vg["img"].cpu(), vh["img"]) and not any(k.startswith("aug_") for k in vg)
    # the grouped training batch: one draw per image slot, applied on the GPU
    ds_h = dh.train_dl.dataset
    np.random.seed(5)
    gb = next(iter(D.DevicePrefetcher([ds.grouped_train_batch([[0, 3], [2, 4]])], "cuda", resize_hw=(64, 96))))
    np.random.seed(5)
    hb = ds_h.grouped_train_batch([[0, 3], [2, 4]])
    torch.cuda.synchronize()
    assert not any(k.startswith("aug_") for k in gb) and set(gb) == set(hb)
    assert torch.equal(gb["img"].cpu(), hb["img"]) and torch.equal(gb["annot"].cpu(), hb["annot"]) and gb["img_idx"].tolist() == [0, 0, 1, 1]


def test_raw_c_abi_argument_errors():
    from zsgnet_pytorch_amd._lib import lib, stream_ptr
    gray = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(120, dtype=torch.uint8, device="cuda")
    fn = lib.zsg_augment_geom_u8_batched
    assert fn(None, None, 1, 24, 32, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert b"augment_geom_u8_batched" in lib.zsg_last_error()
    assert fn(jobs.data_ptr(), None, 0, 24, 32, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert fn(jobs.data_ptr(), None, 1, 0, 32, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert fn(jobs.data_ptr(), None, 1, 24, -1, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert fn(jobs.data_ptr(), None, 1, 24, 32, 0, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert fn(jobs.data_ptr(), None, 1, 24, 32, 1, 3, None, 1, stream_ptr()) == -1
    assert fn(jobs.data_ptr(), None, 1, 5000, 5000, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1      # 32-bit gray sums
    # with the host copy of the table every record is checked: a good record first, then one fault at a time
    a = 1 << 20                                    # (any non-null, dword-aligned number: nothing is launched)
    good = dict(img=a, tmp=a, out=a, xb=a, xc=a, yb=a, yc=a, ih=37, iw=53, wx0=-3, wy0=-2, wh=40, ww=60, xk=9, yk=9, bx=0, by=0, flags=1, fill=0)

    def rec(**kw):
        r = {**good, **kw}
        return struct.pack("<qqqqqqqiiiiiiiiiiiIfffi", r["img"], r["tmp"], r["out"], r["xb"], r["xc"], r["yb"], r["yc"], r["ih"], r["iw"], r["wx0"],
                           r["wy0"], r["wh"], r["ww"], r["xk"], r["yk"], r["bx"], r["by"], r["flags"], r["fill"], 1.0, 1.0, 1.0, 0)

    assert len(rec()) == 120
    bx, by = (40 * 32 + 255) // 256, (24 * 32 + 255) // 256
    for bad in (dict(xb=0), dict(yc=0), dict(img=0), dict(wh=0), dict(ww=-4), dict(ih=0), dict(iw=-1), dict(wh=1 << 16), dict(xk=0), dict(wx0=1 << 25),
                dict(tmp=a + 1), dict(bx=1), dict(by=2)):
        assert fn(jobs.data_ptr(), rec(**bad), 1, 24, 32, bx, by, gray.data_ptr(), 1, stream_ptr()) == -1, bad
        assert b"augment_geom_u8_batched" in lib.zsg_last_error()
    assert fn(jobs.data_ptr(), rec(), 1, 24, 32, bx + 1, by, gray.data_ptr(), 1, stream_ptr()) == -1       # more blocks than the jobs have
    assert fn(jobs.data_ptr(), rec(), 1, 24, 32, bx, by - 1, gray.data_ptr(), 1, stream_ptr()) == -1
    torch.cuda.synchronize()
    assert gray.tolist() == [7, 7, 7, 7]           # nothing was launched (launch 1 would have zeroed the first accumulator)

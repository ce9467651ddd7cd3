"""Training augmentation on the GPU: zsg_augment_u8_batched (csrc/aug.hip) through GpuResizer.resize_flat(..., crop, jitter) against the
byte-exact host definition dat_loader.augment_host (itself pinned to Pillow and to tests/augment_ref.py by tests/test_cpu_augment.py),
then the loader end to end: DevicePrefetcher with gpu_resize against the host-worker path."""
import numpy as np
import pytest
import torch

from zsgnet_pytorch_amd import config, dat_loader as D

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 48), (40, 40), (53, 37), (33, 65), (48, 64)]                      # (h, w)
# whole image | 1 pixel high | 1 pixel wide | smaller than the output (upscales) | inner window | right AND bottom border of the LAST image
CROPS = [(0, 0, 53, 37), (0, 31, 48, 32), (13, 0, 14, 40), (2, 3, 15, 13), (10, 5, 60, 30), (64 - 11, 48 - 9, 64, 48)]
TRIPLES = [(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2), (0.7, 1.3, 0.6)]
OUTS = [(24, 32), (40, 48)]                                                                # (Ho, Wo)


@pytest.fixture(scope="module")
def batch():
    rng = np.random.RandomState(5)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    flat, hw = D.flatten_raw([torch.from_numpy(a) for a in imgs])
    return imgs, flat.cuda(), hw


_REF = {}


def host(imgs, crops, jit, out_hw):
    """augment_host of every job, computed once per (jobs, output size)"""
    key = (tuple(map(tuple, crops)), tuple(map(tuple, np.asarray(jit, np.float32).tolist())), tuple(out_hw), tuple(a.shape for a in imgs))
    if key not in _REF:
        ref = np.stack([D.augment_host(a, c, np.asarray(j, np.float32), out_hw) for a, c, j in zip(imgs, crops, jit)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


@pytest.mark.parametrize("out_hw", OUTS)
def test_resize_flat_with_crop_and_jitter_is_augment_host(batch, out_hw):
    imgs, flat, hw = batch
    rz = D.GpuResizer(out_hw)
    plain = rz.resize_flat(flat, hw)
    for rot in (0, 3):                             # between the two batches every factor triple meets a job
        jit = np.array([TRIPLES[(i + rot) % 8] for i in range(6)], np.float32)
        got = rz.resize_flat(flat, hw, crop=torch.tensor(CROPS, dtype=torch.int32), jitter=torch.from_numpy(jit))
        torch.cuda.synchronize()
        ref = host(imgs, CROPS, jit, out_hw)
        for i in range(6):
            assert np.array_equal(got[i].cpu().numpy(), ref[i]), f"job {i}: {SIZES[i]} window {CROPS[i]} factors {jit[i].tolist()} -> {out_hw}"
        if rot == 0:                               # the whole image with all-ones factors: today's resize, bit for bit
            assert torch.equal(got[0], plain[0])
    # crop alone / jitter alone: the missing one is the whole image / factors 1
    only_crop = rz.resize_flat(flat, hw, crop=CROPS)
    only_jit = rz.resize_flat(flat, hw, jitter=np.ones((6, 3), np.float32))
    torch.cuda.synchronize()
    assert np.array_equal(only_crop.cpu().numpy(), host(imgs, CROPS, np.ones((6, 3)), out_hw)) and torch.equal(only_jit, plain)
    # a window that leaves its image is refused on the host: the kernels read it unchecked
    for bad in ((0, 0, 54, 37), (-1, 0, 5, 5), (5, 5, 5, 9), (0, 30, 5, 38)):
        with pytest.raises(ValueError, match="crop"):
            rz.resize_flat(flat, hw, crop=[bad] + CROPS[1:])
    with pytest.raises(ValueError, match="jitter"):
        rz.resize_flat(flat, hw, jitter=np.full((6, 3), -1.0, np.float32))


def test_skipped_third_launch_repeat_run_and_accumulators(batch):
    imgs, flat, hw = batch
    out_hw = OUTS[0]
    rz = D.GpuResizer(out_hw)
    jit = np.ones((6, 3), np.float32)
    jit[:, 0] = [1, 0, 2, 0.7, 1.3, 0.5]           # contrast and saturation all 1: launch 3 is skipped
    got = rz.resize_flat(flat, hw, crop=CROPS, jitter=jit).clone()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), host(imgs, CROPS, jit, out_hw))
    # the integer gray sums of the jobs: the sum of gray after brightness == channel 0 of the (b, 1, 0) image
    gray = [int(D.augment_host(a, c, np.array([j[0], 1, 0], np.float32), out_hw)[..., 0].astype(np.int64).sum()) for a, c, j in zip(imgs, CROPS, jit)]
    assert rz._gray[:6].tolist() == gray
    full = np.array([TRIPLES[(i + 3) % 8] for i in range(6)], np.float32)
    first = rz.resize_flat(flat, hw, crop=CROPS, jitter=full).clone()
    again = rz.resize_flat(flat, hw, crop=CROPS, jitter=full)
    torch.cuda.synchronize()
    assert torch.equal(first, again) and np.array_equal(again.cpu().numpy(), host(imgs, CROPS, full, out_hw))
    gray = [int(D.augment_host(a, c, np.array([j[0], 1, 0], np.float32), out_hw)[..., 0].astype(np.int64).sum()) for a, c, j in zip(imgs, CROPS, full)]
    assert rz._gray[:6].tolist() == gray, "the accumulators are zeroed by every call, not added to"
    # the device tap-table cache is bounded (crop sides vary per sample)
    rz.TABLE_CACHE = 16
    rng = np.random.RandomState(1)
    for _ in range(6):
        crops = [(x0, y0, x0 + rng.randint(1, w - x0 + 1), y0 + rng.randint(1, h - y0 + 1))
                 for (h, w) in SIZES for x0, y0 in [(rng.randint(0, w), rng.randint(0, h))]]
        got = rz.resize_flat(flat, hw, crop=crops, jitter=full)
        torch.cuda.synchronize()
        assert len(rz._tab) <= 24
        assert np.array_equal(got.cpu().numpy(), host(imgs, crops, full, out_hw))


def test_full_size_batch():
    rng = np.random.RandomState(9)
    cfg = config.get_cfg(aug_crop_min=0.4, aug_brightness=0.4, aug_contrast=0.4, aug_saturation=0.7)
    imgs, crops, jit = [], [], []
    for i in range(16):
        h, w = (375, 500) if i % 3 else (500, 333)
        imgs.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        x1, y1 = rng.uniform(0, w - 40), rng.uniform(0, h - 40)
        c, j = D.draw_augment(rng, h, w, [[x1, y1, x1 + rng.uniform(5, 40), y1 + rng.uniform(5, 40)]], cfg)
        crops.append(c)
        jit.append(j)
    flat, hw = D.flatten_raw([torch.from_numpy(a) for a in imgs])
    got = D.GpuResizer((300, 300)).resize_flat(flat.cuda(), hw, crop=crops, jitter=np.stack(jit))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for i in range(16):
        assert np.array_equal(got[i], D.augment_host(imgs[i], crops[i], jit[i], (300, 300))), f"image {i}: {imgs[i].shape} window {crops[i]} factors {jit[i]}"


def test_loader_end_to_end(tmp_path, gold):
    import PIL.Image
    from zsgnet_pytorch_amd import mdl
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
          "ds_info.refclef.img_dir": str(tmp_path), "ds_info.refclef.trn_csv_file": str(tmp_path / "d.csv"),
          "ds_info.refclef.val_csv_file": str(tmp_path / "d.csv"), "ds_info.refclef.test_csv_file": str(tmp_path / "d.csv")}
    cfg = config.get_cfg(**kw)

    def one_pass(prefetch):
        data = D.get_data(cfg, prefetch=prefetch)
        torch.manual_seed(3)                       # the training loader's shuffle
        np.random.seed(3)                          # the augmentation draws
        return data, [{k: v.cpu() for k, v in b.items()} | {"_dev": b} for b in data.train_dl]

    dg, gpu_batches = one_pass(True)               # raw images + aug_crop / aug_jitter -> DevicePrefetcher -> zsg_augment_u8_batched
    dh, host_batches = one_pass(False)             # augment_host in the (in-process) worker
    torch.cuda.synchronize()
    assert isinstance(dg.train_dl, D.DevicePrefetcher) and dg.train_dl.loader.dataset.gpu_resize and not dh.train_dl.dataset.gpu_resize
    assert len(gpu_batches) == len(host_batches) == 2
    for bg, bh in zip(gpu_batches, host_batches):
        assert not any(k.startswith("aug_") for k in bg) and "img_hw" not in bg
        assert set(bg) == set(bh)
        assert bg["img"].dtype == torch.uint8 and tuple(bg["img"].shape) == (2, 64, 96, 3)
        for k in ("img", "annot", "orig_annot", "img_size", "idxs", "qlens"):
            assert torch.equal(bg[k], bh[k]), k
    # validation batches are never augmented: the same on either path
    vg, vh = next(iter(dg.valid_dl)), next(iter(dh.valid_dl))
    torch.cuda.synchronize()
    assert torch.equal(vg["img"].cpu(), vh["img"]) and "aug_crop" not in vg
    # the grouped training batch: one crop per image slot, applied on the GPU
    ds_g, ds_h = dg.train_dl.loader.dataset, dh.train_dl.dataset
    np.random.seed(5)
    gb = next(iter(D.DevicePrefetcher([ds_g.grouped_train_batch([[0, 3], [2, 4]])], "cuda", resize_hw=(64, 96))))
    np.random.seed(5)
    hb = ds_h.grouped_train_batch([[0, 3], [2, 4]])
    torch.cuda.synchronize()
    assert not any(k.startswith("aug_") for k in gb) and set(gb) == set(hb)
    assert torch.equal(gb["img"].cpu(), hb["img"]) and torch.equal(gb["annot"].cpu(), hb["annot"]) and gb["img_idx"].tolist() == [0, 0, 1, 1]
    # the model sees the keys it always saw
    net = mdl.get_default_net(9, cfg).to("cuda").train()
    dev = gpu_batches[0]["_dev"]
    out = net({**dev, "h0": torch.zeros(2, 2, 128), "c0": torch.zeros(2, 2, 128)})
    torch.cuda.synchronize()
    assert torch.isfinite(out["att_bbx_out"]).all()


def test_raw_c_abi_argument_errors():
    from zsgnet_pytorch_amd._lib import lib, stream_ptr
    gray = torch.zeros(4, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(104, dtype=torch.uint8, device="cuda")
    assert lib.zsg_augment_u8_batched(None, 1, 24, 32, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert b"augment_u8_batched" in lib.zsg_last_error()
    assert lib.zsg_augment_u8_batched(jobs.data_ptr(), 0, 24, 32, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1
    assert lib.zsg_augment_u8_batched(jobs.data_ptr(), 1, 24, 32, 1, 3, None, 1, stream_ptr()) == -1
    assert lib.zsg_augment_u8_batched(jobs.data_ptr(), 1, 5000, 5000, 1, 3, gray.data_ptr(), 1, stream_ptr()) == -1      # 32-bit gray sums
    torch.cuda.synchronize()
    assert gray.tolist() == [0, 0, 0, 0]           # nothing was launched

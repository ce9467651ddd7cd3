"""Developer tool (GPU box): how many images per second the batch producer delivers.
Synthetic JPEGs of photo size (500 x 375) on local disk; compared: (a) the reference's path — PIL decode + PIL resize + float
conversion in the DataLoader workers, (b) this repo's — PIL decode only in the workers, raw uint8 copied to the GPU (pinned, side
stream), zsg_resize_u8 + zsg_u8hwc_to_nhwc4 there.
--aug adds two rows per worker count for the training augmentation (box-safe random crop + colour jitter, cfg aug_*): (c) on the GPU —
the workers draw the crop and the factors, the raw image travels as in (b), zsg_augment_u8_batched crops, resizes and jitters — and
(d) in the workers (dat_loader.augment_host: what the loader does without gpu_img_resize), uint8 300 x 300 uploaded.
--flip P and / or --expand R (with --aug) add the same two rows with aug_flip = P / aug_expand_max = R on top (dat_loader.draw_augment_geom;
on the GPU zsg_augment_geom_u8_batched whenever a job of the batch is flipped or its window leaves the image).  After the rows --aug
prints the DEVICE time of the augmentation launches for one batch of 16 (the library's own HIP events around each entry point's
launches, median of 20 calls), per configuration.
--rotate D / --shear D / --blur S (with --aug) likewise put aug_rotate / aug_shear / aug_blur on top (dat_loader.draw_augment_warp; on the
GPU zsg_augment_warp_u8_batched after the other entry, whenever a job of the batch is warped or blurred: its device time is printed on a
line of its own).
usage: python tools/loader_rate.py [--aug [--flip P] [--expand R] [--rotate D] [--shear D] [--blur S]] [n_images] [workers ...]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import dat_loader as D
from zsgnet_pytorch_amd._lib import lib, check, stream_ptr, ProfEntry


AUG_CFG = {"aug_crop_min": 0.5, "aug_brightness": 0.4, "aug_contrast": 0.4, "aug_saturation": 0.4}
FILL = (124, 116, 104)


def draw(i, h, w, cfg):
    """the augmentation of image i: (crop, jitter, flip, six warp integers, sigma), from a generator seeded by i (with the warp / blur keys
    off draw_augment_warp draws draw_augment_geom's numbers; then the identity and 0)"""
    rng = np.random.RandomState(i)
    x1, y1 = rng.uniform(0, w - 120), rng.uniform(0, h - 120)
    crop, jit, flip, warp, sigma = D.draw_augment_warp(rng, h, w, [[x1, y1, x1 + rng.uniform(20, 120), y1 + rng.uniform(20, 120)]], cfg, (300, 300))
    return crop, jit, flip, D.warp_matrix(*warp, (300, 300)) if warp is not None else D.WARP_IDENTITY, sigma or 0.0


class Raw(torch.utils.data.Dataset):
    def __init__(self, files, resize, aug=None, cfg=AUG_CFG):
        """aug: None, "gpu" (the item carries the drawn crop / factors) or "host" (the worker applies them: augment_host); cfg: the aug_*
        keys (AUG_CFG, or with aug_flip / aug_expand_max / aug_rotate / aug_shear / aug_blur on top: the item then carries aug_geom too, and
        with one of the last three aug_warp and aug_blur)"""
        self.files, self.resize, self.aug, self.cfg = files, resize, aug, cfg
        self.geom = cfg is not AUG_CFG
        self.warp = D.aug_warp_enabled(cfg)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        import PIL.Image
        img = PIL.Image.open(self.files[i]).convert("RGB")
        if self.aug:
            crop, jit, flip, warp, sigma = draw(i, img.height, img.width, self.cfg)
            if self.aug == "host":
                return torch.from_numpy(D.augment_host(np.asarray(img), crop, jit, (300, 300), flip=flip, fill=FILL if self.geom else None, warp=warp, blur=sigma))
            item = {"img": torch.from_numpy(np.asarray(img).copy()), "aug_crop": torch.tensor(crop, dtype=torch.int32), "aug_jitter": torch.from_numpy(jit)}
            if self.geom:
                item["aug_geom"] = torch.tensor([int(flip), *FILL], dtype=torch.int32)
            if self.warp:
                item["aug_warp"], item["aug_blur"] = torch.tensor(warp, dtype=torch.int32), torch.tensor(sigma, dtype=torch.float32)
            return item
        if self.resize:                                             # the reference's item: resize + float conversion on the host
            img = img.resize((300, 300))
            return torch.from_numpy(np.asarray(img).transpose(2, 0, 1).astype(np.float64)).float().div_(255)
        return torch.from_numpy(np.asarray(img).copy())             # raw uint8 [h, w, 3]


def collate_raw(b):
    if isinstance(b[0], dict):                                          # GPU augmentation: raw images + one crop / factor triple each
        out = dict(zip(("img", "img_hw"), D.flatten_raw([x["img"] for x in b])))
        for k in ("aug_crop", "aug_jitter", "aug_geom", "aug_warp", "aug_blur"):
            if k in b[0]:
                out[k] = torch.stack([x[k] for x in b])
        return out
    return dict(zip(("img", "img_hw"), D.flatten_raw(b)))


def device_time(files, cfg, label, calls=20, warmup=5):
    """one batch of 16 through GpuResizer.resize_flat: the device time between the first and the last launch of the entry point"""
    import PIL.Image
    imgs = [np.asarray(PIL.Image.open(f).convert("RGB")) for f in files[:16]]
    draws = [draw(i, a.shape[0], a.shape[1], cfg) for i, a in enumerate(imgs)]
    flat, hw = D.flatten_raw([torch.from_numpy(a.copy()) for a in imgs])
    flat = flat.cuda()
    geom = cfg is not AUG_CFG
    kw = dict(crop=[d[0] for d in draws], jitter=np.stack([d[1] for d in draws]))
    if geom:
        kw.update(flip=[d[2] for d in draws], fill=FILL)
    if D.aug_warp_enabled(cfg):
        kw.update(warp=[d[3] for d in draws], blur=[d[4] for d in draws])
    rz = D.GpuResizer((300, 300))
    ents, ms = (ProfEntry * 16)(), {}
    lib.zsg_prof_enable(1)
    try:
        for i in range(warmup + calls):
            lib.zsg_prof_collect(ents, 16)                              # (drop earlier records)
            rz.resize_flat(flat, hw, **kw)
            n = lib.zsg_prof_collect(ents, 16)                          # (waits for the recorded events)
            if i >= warmup:
                for e in ents[:n]:
                    ms.setdefault(e.name.decode(), []).append(e.ms)
    finally:
        lib.zsg_prof_enable(0)
    rows = sum(d[0][3] - d[0][1] for d in draws)
    for name, v in ms.items():
        print(f"  device time, batch of 16  {label:34s} {name:18s} median {1e3 * np.median(v):7.1f} us  (min {1e3 * min(v):.1f}, max {1e3 * max(v):.1f}; "
              f"{rows} window rows in launch 1, {sum(bool(d[2]) for d in draws)} flipped, {sum(d[3] != D.WARP_IDENTITY for d in draws)} warped, "
              f"{sum(bool(d[4]) for d in draws)} blurred)")


def main():
    import PIL.Image
    argv, geom_cfg = [], dict(AUG_CFG)
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--flip":
            geom_cfg["aug_flip"] = float(next(it))
        elif a == "--expand":
            geom_cfg["aug_expand_max"] = float(next(it))
        elif a in ("--rotate", "--shear", "--blur"):
            geom_cfg["aug_" + a[2:]] = float(next(it))
        elif a != "--aug":
            argv.append(a)
    geom = len(geom_cfg) > len(AUG_CFG)
    if geom and "--aug" not in sys.argv:
        sys.exit("--flip / --expand / --rotate / --shear / --blur need --aug")
    D.aug_geom_params(geom_cfg)                                         # ValueError outside the keys' ranges
    D.aug_warp_params(geom_cfg)
    n = int(argv[0]) if argv else 512
    workers = [int(a) for a in argv[1:]] or [1, 4, 16]
    rng = np.random.default_rng(0)
    td = tempfile.mkdtemp()
    files = []
    for i in range(64):
        h, w = (375, 500) if i % 3 else (500, 333)
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.clip(127 + 90 * np.sin(yy / 17.0 + i)[..., None] * np.cos(xx / 23.0)[..., None] * np.array([1, .6, -.7]) + rng.normal(0, 12, (h, w, 3)), 0, 255)
        f = os.path.join(td, f"{i}.jpg")
        PIL.Image.fromarray(a.astype(np.uint8)).save(f, quality=90)
        files.append(f)
    files = (files * ((n + 63) // 64))[:n]
    print(f"{n} JPEGs (500x375 / 333x500), batch 16 -> 300x300; images per second")
    geom_tag = " ".join(f"{k[4:]} {v:g}" for k, v in geom_cfg.items() if k not in AUG_CFG)
    for nw in workers:
        modes = ["host resize (reference path)", "GPU resize (zsg_resize_u8)"]
        if "--aug" in sys.argv:
            modes += ["GPU augment (zsg_augment_u8)", "host-worker augment (augment_host)"]
        if geom:
            modes += [f"GPU augment + {geom_tag}", f"host-worker augment + {geom_tag}"]
        for mode in modes:
            host = mode.startswith("host")
            ds = Raw(files, resize=host, aug=("gpu" if mode.startswith("GPU augment") else "host" if mode.startswith("host-worker") else None),
                     cfg=geom_cfg if "+" in mode else AUG_CFG)
            dl = torch.utils.data.DataLoader(ds, batch_size=16, num_workers=nw, pin_memory=True, persistent_workers=False,
                                             collate_fn=(None if host else collate_raw))
            it = dl if host else D.DevicePrefetcher(dl, "cuda", resize_hw=(300, 300))      # (side-stream copies + resize, as the trainer's loader)
            t0, cnt = None, 0
            for bi, b in enumerate(it):
                if bi == 2:
                    torch.cuda.synchronize()
                    t0, cnt = time.perf_counter(), 0
                if host and b.dtype == torch.uint8:                    # augmented in the workers: uint8 HWC at the final size
                    u8 = b.cuda(non_blocking=True)
                    out = torch.empty(u8.shape[0], 300, 300, 4, device="cuda")
                    check(lib.zsg_u8hwc_to_nhwc4(u8.data_ptr(), u8.shape[0] * 300 * 300, out.data_ptr(), stream_ptr()), "u8")
                    cnt += u8.shape[0]
                elif host:
                    x = b.cuda(non_blocking=True)
                    cnt += x.shape[0]
                else:
                    u8 = b["img"]
                    out = torch.empty(u8.shape[0], 300, 300, 4, device="cuda")
                    check(lib.zsg_u8hwc_to_nhwc4(u8.data_ptr(), u8.shape[0] * 300 * 300, out.data_ptr(), stream_ptr()), "u8")
                    cnt += u8.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"  workers {nw:2d}  {mode:44s} {cnt / dt:8.1f} img/s  ({cnt / dt / nw:7.1f} per worker)")
    if "--aug" in sys.argv:
        device_time(files, AUG_CFG, "GPU augment")
        if geom:
            device_time(files, geom_cfg, f"GPU augment + {geom_tag}")


if __name__ == "__main__":
    main()

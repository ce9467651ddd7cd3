"""Rotation / shear and Gaussian blur of the training augmentation on the GPU: zsg_augment_warp_u8_batched (csrc/aug.hip) through
GpuResizer.resize_flat(..., warp, blur) against the byte-exact host definition dat_loader.augment_host(..., warp, blur) (itself pinned by
tests/test_cpu_augment_warp.py) — byte equality everywhere, no tolerance — then the C entry's argument checks and the loader end to end."""
import struct

import numpy as np
import pytest
import torch

from zsgnet_pytorch_amd import config, dat_loader as D

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 48), (30, 40)]             # (h, w): 5883 and 9216 bytes, so the second and third image start off a dword boundary
OUTS = [(24, 32), (40, 48), (25, 31)]              # (Ho, Wo): whole blocks | a partial last block | odd width, 93-byte rows, a byte tail
TRIPLES = [(1, 1, 1), (0.7, 1.3, 0.6), (2, 1, 1), (1, 0, 1), (1, 1, 2)]
FILL = (124, 116, 104)
ID = D.WARP_IDENTITY
SENTINEL = 0xA5
# (theta, shear) or None, sigma: identity | warp only: both signs, theta alone, shear alone | blur only | both
KINDS = [(None, 0.0), ((15.0, 8.0), 0.0), ((-15.0, -8.0), 0.0), ((15.0, -8.0), 0.0), ((12.0, 0.0), 0.0), ((0.0, -8.0), 0.0),
         (None, 0.1), (None, 0.3), (None, 1.0), (None, 2.5), ((15.0, 8.0), 1.0), ((-7.5, 3.0), 2.5), ((30.0, 20.0), 0.3)]


@pytest.fixture(scope="module")
def batch():
    """39 jobs: every job kind on each of the three images"""
    rng = np.random.RandomState(5)
    three = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    imgs = three * len(KINDS)
    flat, hw = D.flatten_raw([torch.from_numpy(a) for a in imgs])
    return imgs, flat.cuda(), hw


def jobs_for(out_hw, geom):
    """geom: the jobs also carry crop windows that leave the image, jitter triples and flips, so the geom path feeds the new launches"""
    n = 3 * len(KINDS)
    warps = [D.warp_matrix(*KINDS[i // 3][0], out_hw) if KINDS[i // 3][0] is not None else ID for i in range(n)]
    blurs = [float(np.float32(KINDS[i // 3][1])) for i in range(n)]                         # (float32: what a batch's aug_blur field carries)
    fills = np.array([FILL if i % 5 else (0, 255, 7) for i in range(n)], np.int32)        # a non-grey fill on every fifth job
    if not geom:
        return None, None, None, fills, warps, blurs
    h_w = [SIZES[i % 3] for i in range(n)]
    wins = [[(0, 0, w, h), (2, 3, 15, 13), (-5, -4, w - 3, h - 2), (4, 3, w + 7, h + 6), (-w - 5, -(h // 2), 2 * w - 5, 3 * h - h // 2)][(i + i // 3) % 5]
            for i, (h, w) in enumerate(h_w)]
    jit = np.array([TRIPLES[(i + 1) % 5] for i in range(n)], np.float32)
    flips = [bool((i + i // 3) % 2) for i in range(n)]
    return wins, jit, flips, fills, warps, blurs


_REF = {}


def host(imgs, out_hw, geom):
    """augment_host of every job, computed once per (output size, geom) and kept read-only"""
    if (out_hw, geom) not in _REF:
        wins, jit, flips, fills, warps, blurs = jobs_for(out_hw, geom)
        ref = np.stack([D.augment_host(a, wins[i] if geom else (0, 0, a.shape[1], a.shape[0]), jit[i] if geom else np.ones(3, np.float32), out_hw,
                                       flip=flips[i] if geom else False, fill=tuple(int(v) for v in fills[i]), warp=warps[i], blur=blurs[i])
                        for i, a in enumerate(imgs)])
        ref.setflags(write=False)
        _REF[(out_hw, geom)] = ref
    return _REF[(out_hw, geom)]


def assert_jobs_equal(got, ref, out_hw):
    got = got.cpu().numpy()
    for i in range(len(ref)):
        assert np.array_equal(got[i], ref[i]), f"job {i}: {SIZES[i % 3]} kind {KINDS[i // 3]} -> {out_hw}: {int((got[i] != ref[i]).sum())} bytes differ"


@pytest.mark.parametrize("geom", [False, True], ids=["plain resize", "crop + jitter + flip"])
@pytest.mark.parametrize("out_hw", OUTS)
def test_resize_flat_with_warp_and_blur_is_augment_host(batch, out_hw, geom):
    imgs, flat, hw = batch
    rz = D.GpuResizer(out_hw)
    wins, jit, flips, fills, warps, blurs = jobs_for(out_hw, geom)
    n = len(imgs)
    buf = torch.full((n + 2, out_hw[0], out_hw[1], 3), SENTINEL, dtype=torch.uint8, device="cuda")      # one image of sentinels in front and behind
    got = rz.resize_flat(flat, hw, out=buf[1:n + 1], crop=wins, jitter=jit, flip=flips, fill=torch.from_numpy(fills),
                         warp=torch.tensor(warps, dtype=torch.int32), blur=torch.tensor(blurs, dtype=torch.float32))
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[1].data_ptr() and rz.warp_calls == 1
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[n + 1] == SENTINEL).all()), "a store left [B, Ho, Wo, 3]"
    ref = host(imgs, out_hw, geom)
    assert_jobs_equal(got, ref, out_hw)
    assert rz.launches["augment_geom_u8"] == int(geom), "flips and windows that leave the image: the geom entry feeds the new launches"
    # the scratch batch holds the un-warped result, untouched: the source is never written
    plain = rz.resize_flat(flat, hw, crop=wins, jitter=jit, flip=flips, fill=torch.from_numpy(fills) if geom else None)
    torch.cuda.synchronize()
    assert torch.equal(rz._warp_src[:n], plain) and rz.warp_calls == 1
    # a second call gives the same bytes (nothing accumulates), also into a fresh tensor
    again = rz.resize_flat(flat, hw, crop=wins, jitter=jit, flip=flips, fill=fills, warp=warps, blur=blurs)
    torch.cuda.synchronize()
    assert torch.equal(again, got) and rz.warp_calls == 2


@pytest.mark.parametrize("out_hw", OUTS)
def test_single_stages_and_one_job_among_identities(batch, out_hw):
    imgs, flat, hw = batch
    n = len(imgs)
    rz = D.GpuResizer(out_hw)
    _, _, _, fills, warps, blurs = jobs_for(out_hw, False)
    base = rz.resize_flat(flat, hw).clone()
    torch.cuda.synchronize()
    base_np = base.cpu().numpy()
    # warp launch only (no scratch for the blur is allocated), blur launches only (no fill needed)
    only_w = rz.resize_flat(flat, hw, fill=fills, warp=warps)
    torch.cuda.synchronize()
    assert rz._warp_tmp is None
    for i in range(n):
        assert np.array_equal(only_w[i].cpu().numpy(), D.warp_host(base_np[i], warps[i], fills[i].tolist())), i
    only_b = rz.resize_flat(flat, hw, blur=blurs)
    torch.cuda.synchronize()
    for i in range(n):
        assert np.array_equal(only_b[i].cpu().numpy(), D.blur_host(base_np[i], blurs[i]) if blurs[i] else base_np[i]), i
    # a single warped job among identities; a single blurred one
    for k, (w, b) in ((4, (D.warp_matrix(-15.0, 8.0, out_hw), 0.0)), (n - 1, (ID, 2.5)), (0, (D.warp_matrix(5.0, 0.0, out_hw), 0.5))):
        ws, bs = [ID] * n, [0.0] * n
        ws[k], bs[k] = w, b
        got = rz.resize_flat(flat, hw, fill=FILL, warp=ws, blur=bs)
        torch.cuda.synchronize()
        want = D.augment_host(imgs[k], (0, 0, imgs[k].shape[1], imgs[k].shape[0]), np.ones(3, np.float32), out_hw, fill=FILL, warp=w, blur=b)
        assert np.array_equal(got[k].cpu().numpy(), want)
        rest = [i for i in range(n) if i != k]
        assert torch.equal(got[rest], base[rest]), "the other jobs pass through unchanged"
    with pytest.raises(ValueError, match="fill"):
        rz.resize_flat(flat, hw, warp=warps)
    with pytest.raises(ValueError, match="warp must be"):
        rz.resize_flat(flat, hw, fill=FILL, warp=warps[:-1])
    with pytest.raises(ValueError, match="blur"):
        rz.resize_flat(flat, hw, blur=[-1.0] * n)
    with pytest.raises(ValueError, match="32 bits"):
        rz.resize_flat(flat, hw, fill=FILL, warp=[(1 << 31, 0, 0, 0, 65536, 0)] * n)


def test_right_angle_rotations_of_a_square_output(batch):
    imgs, flat, hw = batch
    n = 16
    rz = D.GpuResizer((n, n))
    base = rz.resize_flat(flat[:37 * 53 * 3 + 64 * 48 * 3], hw[:2]).clone()
    r90 = (0, 65536, 0, -65536, 0, (n - 1) * 65536)
    r180 = (-65536, 0, (n - 1) * 65536, 0, -65536, (n - 1) * 65536)
    got = rz.resize_flat(flat[:37 * 53 * 3 + 64 * 48 * 3], hw[:2], fill=(1, 2, 3), warp=[r90, r180])
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), np.rot90(base[0].cpu().numpy(), 3))
    assert np.array_equal(got[1].cpu().numpy(), np.rot90(base[1].cpu().numpy(), 2))
    # coefficients near the ends of 32 bits: the sums are taken in 64 bits (the host's int64), far-away taps are fill
    far = [(2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1, 0, 0, 65536, 0)]
    got = rz.resize_flat(flat[:37 * 53 * 3 + 64 * 48 * 3], hw[:2], fill=(1, 2, 3), warp=far)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(got[i].cpu().numpy(), D.warp_host(base[i].cpu().numpy(), far[i], (1, 2, 3))), i


@pytest.mark.parametrize("out_hw", OUTS)
def test_a_batch_without_warp_or_blur_takes_todays_path(batch, out_hw):
    imgs, flat, hw = batch
    n = len(imgs)
    wins, jit, flips, fills, _, _ = jobs_for(out_hw, True)
    rz, rz0 = D.GpuResizer(out_hw), D.GpuResizer(out_hw)
    before = rz0.resize_flat(flat, hw, crop=wins, jitter=jit, flip=flips, fill=fills)
    got = rz.resize_flat(flat, hw, crop=wins, jitter=jit, flip=flips, fill=fills, warp=[ID] * n, blur=[0.0] * n)
    plain0 = rz0.resize_flat(flat, hw)
    plain = rz.resize_flat(flat, hw, warp=torch.tensor([ID] * n, dtype=torch.int32), blur=torch.zeros(n))
    inside0 = rz0.resize_flat(flat, hw, jitter=jit)
    inside = rz.resize_flat(flat, hw, jitter=jit, blur=[0.0] * n)
    torch.cuda.synchronize()
    assert torch.equal(got, before) and torch.equal(plain, plain0) and torch.equal(inside, inside0)
    assert rz.warp_calls == 0 and rz._warp_src is None and rz._warp_tmp is None, "no call of the new entry, nothing new allocated"
    assert rz.launches == rz0.launches == {"augment_u8": 1, "augment_geom_u8": 1}


def test_raw_c_abi_argument_errors():
    """argument checks only: every call returns -1 before anything is launched, and the output buffer keeps its sentinel"""
    from zsgnet_pytorch_amd._lib import lib, stream_ptr
    Ho, Wo, per = 24, 32, 24 * 32 * 3
    src = torch.full((2, Ho, Wo, 3), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((2, Ho, Wo, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    tmp = torch.full((2 * per,), SENTINEL, dtype=torch.uint8, device="cuda")
    table = torch.zeros(256, dtype=torch.uint8, device="cuda")
    fn = lib.zsg_augment_warp_u8_batched
    taps1 = [16384, 32768, 16384]

    def rec(i, src_p=None, out_p=None, m=ID, fill=0, flags=3, radius=1, taps=taps1):
        return struct.pack("<qq6iIii17i2i", src.data_ptr() + i * per if src_p is None else src_p, out.data_ptr() + i * per if out_p is None else out_p,
                           *m, fill, flags, radius, *(list(taps) + [0] * (17 - len(taps))), 0, 0)

    good = rec(0) + rec(1)
    assert len(good) == 256
    args = dict(dev=table.data_ptr(), host=good, n=2, Ho=Ho, Wo=Wo, tmp=tmp.data_ptr(), stages=3)

    def call(**kw):
        a = {**args, **kw}
        return fn(a["dev"], a["host"], a["n"], a["Ho"], a["Wo"], a["tmp"], a["stages"], stream_ptr())

    bad_calls = [dict(dev=None), dict(dev=table.data_ptr() + 4), dict(n=0), dict(Ho=0), dict(Wo=-1), dict(Ho=1 << 16), dict(stages=0), dict(stages=4),
                 dict(tmp=None), dict(tmp=tmp.data_ptr() + 1),
                 dict(host=rec(0, radius=9) + rec(1)), dict(host=rec(0) + rec(1, radius=-1)),                      # radius outside 0..8
                 dict(host=rec(0, taps=[16384, 32767, 16384]) + rec(1)),                                           # the taps sum to 65535
                 dict(host=rec(0) + rec(1, taps=[-1, 65538, -1])),                                                 # negative taps
                 dict(host=rec(0, radius=8, taps=[3855] * 17) + rec(1)),                                           # 65535 over 17 taps
                 dict(host=rec(0, out_p=src.data_ptr()) + rec(1)),                                                 # out is the source
                 dict(host=rec(0, out_p=src.data_ptr() + per) + rec(1)),                                           # out is another job's source
                 dict(host=rec(0, out_p=tmp.data_ptr()) + rec(1, out_p=tmp.data_ptr() + per)),                     # out is the scratch
                 dict(host=rec(0, src_p=0) + rec(1)), dict(host=rec(0) + rec(1, out_p=0)),                         # null addresses
                 dict(host=rec(0, flags=4) + rec(1)), dict(host=rec(0, flags=-1) + rec(1)), dict(host=rec(0, fill=1 << 24) + rec(1)),
                 dict(host=rec(0, flags=1) + rec(1, flags=1), stages=2, tmp=tmp.data_ptr()),                       # a warp job, no warp launch
                 dict(host=rec(0, flags=2) + rec(1, flags=0), stages=1)]                                           # a blur job, no blur launches
    for bad in bad_calls:
        assert call(**bad) == -1, {k: v for k, v in bad.items() if k != "host"}
        assert b"augment_warp_u8_batched" in lib.zsg_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((tmp == SENTINEL).all()) and bool((src == 9).all()), "nothing was launched"


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
          "aug_rotate": 15.0, "aug_shear": 8.0, "aug_blur": 2.0, "aug_blur_p": 0.6,
          "ds_info.refclef.img_dir": str(tmp_path), "ds_info.refclef.trn_csv_file": str(tmp_path / "d.csv"),
          "ds_info.refclef.val_csv_file": str(tmp_path / "d.csv"), "ds_info.refclef.test_csv_file": str(tmp_path / "d.csv")}
    raw = {str(n): g["png_" + str(n)[0]] for n in g["csv_img"]}

    def one_pass(cfg, prefetch, seed):
        data = D.get_data(cfg, prefetch=prefetch)
        torch.manual_seed(seed)                    # the training loader's shuffle
        np.random.seed(seed)                       # the augmentation draws
        return data, [{k: v.cpu() for k, v in b.items()} for b in data.train_dl]

    for extra, seed in (({}, 3), ({"aug_flip": 0.0, "aug_expand_max": 1.0, "aug_crop_min": 1.0, "aug_brightness": 0.0, "aug_contrast": 0.0, "aug_saturation": 0.0}, 4)):
        cfg = config.get_cfg(**{**kw, **extra})    # every key on | the new keys alone (whole-image windows, factors 1 feed the new launches)
        dg, gpu_batches = one_pass(cfg, True, seed)     # raw images + aug_* fields -> DevicePrefetcher -> the GPU
        dh, host_batches = one_pass(cfg, False, seed)   # augment_host in the (in-process) worker
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
        np.random.seed(seed)
        order = [int(i) for b in gpu_batches for i in b["idxs"]]                           # (nw = 0: the items were drawn in this order)
        stages = set()
        for pos, i in enumerate(order):
            it = ds[i]
            flip, fill = bool(it["aug_geom"][0]), tuple(it["aug_geom"][1:].tolist())
            assert fill == (10, 200, 30)
            m, sigma = tuple(it["aug_warp"].tolist()), float(it["aug_blur"])
            stages |= {"warp"} if m != ID else set()
            stages |= {"blur"} if sigma else set()
            want = D.augment_host(raw[str(g["csv_img"][i])], it["aug_crop"].tolist(), it["aug_jitter"].numpy(), (64, 96), flip=flip, fill=fill, warp=m, blur=sigma)
            assert np.array_equal(gpu_batches[pos // 2]["img"][pos % 2].numpy(), want), (pos, i)
            assert torch.equal(gpu_batches[pos // 2]["orig_annot"][pos % 2], it["orig_annot"])
        assert stages == {"warp", "blur"}, "the seed exercises both stages"
        assert 1 <= dg.train_dl._resizer.warp_calls <= 2
        # validation batches are never augmented: the same on either path
        vg, vh = next(iter(dg.valid_dl)), next(iter(dh.valid_dl))
        torch.cuda.synchronize()
        assert torch.equal(vg["img"].cpu(), vh["img"]) and not any(k.startswith("aug_") for k in vg)
        assert dg.valid_dl._resizer is None or dg.valid_dl._resizer.warp_calls == 0
    # the grouped training batch: one draw per image slot, applied on the GPU
    ds_h = dh.train_dl.dataset
    np.random.seed(5)
    gb = next(iter(D.DevicePrefetcher([ds.grouped_train_batch([[0, 3], [2, 4]])], "cuda", resize_hw=(64, 96))))
    np.random.seed(5)
    hb = ds_h.grouped_train_batch([[0, 3], [2, 4]])
    torch.cuda.synchronize()
    assert not any(k.startswith("aug_") for k in gb) and set(gb) == set(hb)
    assert torch.equal(gb["img"].cpu(), hb["img"]) and torch.equal(gb["annot"].cpu(), hb["annot"]) and gb["img_idx"].tolist() == [0, 0, 1, 1]

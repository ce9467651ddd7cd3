"""The grouped TRAINING loader (cfg group_trn_by_image / trn_queries_per_image): dat_loader.GroupedTrainSampler on a synthetic file
list, ImgQuDataset.grouped_train_batch + grouped_collater on the g13_dataset fixture, and
synth.SyntheticLoader's grouped batches."""
import numpy as np
import pytest
import torch

from zsgnet_pytorch_amd import config, dat_loader as D, synth

# 7 files with 1 .. 9 rows each, shuffled as a CSV would list them: 36 rows, 12 chunks of 4 (1 + 1 + 2 + 2 + 3 + 1 + 2)
COUNTS = {"a": 1, "b": 4, "c": 5, "d": 8, "e": 9, "f": 2, "g": 7}


def file_list():
    rows = [f for f, n in COUNTS.items() for _ in range(n)]
    rng = np.random.default_rng(0)
    rng.shuffle(rows)
    return rows


def n_chunks(k):
    return sum(-(-n // k) for n in COUNTS.values())


@pytest.mark.parametrize("world", [1, 2])
def test_batches_slots_coverage_and_redraws(world):
    files, bs, k = file_list(), 8, 4
    assert n_chunks(k) == 12                                 # 1+1+2+2+3+1+2: divides by world * bs / k, so nothing is dropped
    seen, counts = set(), []
    for rank in range(world):
        s = D.GroupedTrainSampler(files, bs, k, rank, world)
        bts = s.batches(0)
        counts.append(len(bts))
        assert len(bts) == len(s) == 12 // (world * 2)
        for b in bts:
            assert len(b) == bs // k and sum(len(c) for c in b) == bs          # bs // k slots, bs queries, every slot used
            for ch in b:
                assert len(ch) == k and len({files[r] for r in ch}) == 1, "a chunk (re-drawn rows included) stays inside one file"
                seen.update(ch)
    assert len(set(counts)) == 1, "ranks get equal batch counts"
    assert seen == set(range(len(files))), "every dataset row appears at least once per epoch across the ranks"


def test_epochs_differ_and_repeat():
    files = file_list()
    s = D.GroupedTrainSampler(files, 8, 4)
    e0, e1 = s.batches(0), s.batches(1)
    assert e0 != e1, "two epochs must differ"
    assert D.GroupedTrainSampler(files, 8, 4).batches(0) == e0, "the same (seed, epoch) repeats"
    assert D.GroupedTrainSampler(files, 8, 4, seed=5).batches(0) != e0
    it0 = list(s)                       # iterating advances the epoch by itself; set_epoch pins it
    it1 = list(s)
    assert it0 == e0 and it1 == e1
    s.set_epoch(0)
    assert list(s) == e0
    # all ranks cut the same shuffled chunk list
    a, b = D.GroupedTrainSampler(files, 8, 4, 0, 2), D.GroupedTrainSampler(files, 8, 4, 1, 2)
    assert a.chunks(3) == b.chunks(3)
    assert [c for bt in a.batches(3) for c in bt] == a.chunks(3)[0::2][:len(a) * 2]
    assert [c for bt in b.batches(3) for c in bt] == a.chunks(3)[1::2][:len(b) * 2]


def test_short_last_batch_is_dropped_and_bad_sizes_raise():
    files = file_list()
    s = D.GroupedTrainSampler(files, 12, 4)                  # 12 chunks -> 4 batches of 3
    assert len(s) == 4
    s = D.GroupedTrainSampler(files, 20, 4)                  # 12 chunks -> 2 batches of 5, 2 chunks dropped
    assert len(s) == 2 and all(len(b) == 5 for b in s.batches(0))
    for bs, k in ((10, 4), (2, 4), (8, 0)):
        with pytest.raises(ValueError):
            D.GroupedTrainSampler(files, bs, k)
    with pytest.raises(ValueError):
        synth.SyntheticLoader(config.get_cfg(), 10, 2, group_k=4)


@pytest.fixture()
def tiny(tmp_path, gold):
    """15 rows over the three images of g13, interleaved, as tests/test_cpu_grouped_loader.py builds them"""
    import PIL.Image
    g = gold("g13_dataset")
    for k in "abc":
        PIL.Image.fromarray(g["png_" + k]).save(tmp_path / f"{k}.png")
    rows = list(zip(g["csv_img"], g["csv_bbox"], g["csv_query"]))
    names = sorted({str(r[0]) for r in rows})
    with open(tmp_path / "d.csv", "w") as f:
        f.write("img_id,bbox,query\n")
        for n in range(15):
            _, b, q = rows[n % len(rows)]
            f.write(f'{names[(2 * n + n // 7) % len(names)]},"{[float(v) + n % 3 for v in b]}","{q}"\n')
    np.savez(tmp_path / "vec.npz", words=g["words"], vectors=g["table"])
    cfg = config.get_cfg(resize_img=[int(v) for v in g["resize_img"]], word_vectors=str(tmp_path / "vec.npz"), ds_to_use="refclef", bs=6, nw=0,
                         group_trn_by_image=True, trn_queries_per_image=2,
                         **{"ds_info.refclef.img_dir": str(tmp_path), "ds_info.refclef.trn_csv_file": str(tmp_path / "d.csv")})
    return cfg, tmp_path


def test_dataset_batches_and_collater_checks(tiny):
    cfg, root = tiny
    ds = D.ImgQuDataset(cfg, root / "d.csv", "refclef", gpu_normalise=True)
    per_file = {}
    for f in ds.files:
        per_file[f] = per_file.get(f, 0) + 1
    chunks = sum(-(-n // 2) for n in per_file.values())
    decoded = []
    load = ds.load_image
    ds.load_image = lambda idx: (decoded.append(ds.files[idx]), load(idx))[1]
    dl = D.get_dataloader(cfg, ds, is_train=True)
    assert isinstance(dl.sampler, D.GroupedTrainSampler) and len(dl) == chunks // 3
    seen, n = set(), 0
    for bt in dl:
        n += 1
        assert bt["img"].shape[0] == 3 and bt["qvec"].shape[0] == 6 and bt["img_idx"].dtype == torch.long
        assert bt["img_idx"].tolist() == [0, 0, 1, 1, 2, 2], "one slot per chunk, every slot used, equal groups"
        rows = [int(i) for i in bt["idxs"].tolist()]
        seen.update(rows)
        for s_ in range(3):
            assert len({ds.files[rows[2 * s_]], ds.files[rows[2 * s_ + 1]]}) == 1, "the queries of a slot share its image file"
    assert n == len(dl) and len(decoded) == 3 * n, "each slot's image is decoded once"
    if chunks % 3 == 0:
        assert seen == set(range(15))
    ds.load_image = load
    # two chunks of ONE file in a batch still take two slots
    f0 = [i for i, f in enumerate(ds.files) if f == ds.files[0]]
    f1 = [i for i, f in enumerate(ds.files) if f != ds.files[0]]
    bt = ds.grouped_train_batch([f0[:2], f0[2:4]])
    assert bt["img"].shape[0] == 2 and bt["img_idx"].tolist() == [0, 0, 1, 1] and torch.equal(bt["img"][0], bt["img"][1])
    with pytest.raises(ValueError):
        ds.grouped_train_batch([[f0[0], f1[0]]])             # rows of two files in one chunk
    img, h, w = ds.load_image(0)
    items = [ds.query_item(f0[0], h, w), ds.query_item(f0[1], h, w)]
    with pytest.raises(ValueError, match="used by no query"):
        D.grouped_collater(items, [img, img], [0, 0], all_slots_used=True)
    D.grouped_collater(items, [img, img], [0, 0])            # (the validation loader does not ask for it)
    with pytest.raises(ValueError):
        D.grouped_collater(items, [img], [0, 1], all_slots_used=True)


def test_synthetic_loader_yields_grouped_training_batches():
    cfg = config.get_cfg(bs=8, steps_per_epoch=3, resize_img=[32, 32], group_trn_by_image=True, trn_queries_per_image=4)
    dw = synth.get_data(cfg)
    bts = list(dw.train_dl)
    assert len(bts) == 3
    for bt in bts:
        assert bt["img"].shape[0] == 2 and bt["qvec"].shape[0] == 8
        assert sorted(bt["img_idx"].tolist()) == [0] * 4 + [1] * 4
    assert "img_idx" not in next(iter(dw.valid_dl))
    cfg = config.get_cfg(bs=8, steps_per_epoch=2, resize_img=[32, 32])
    assert "img_idx" not in next(iter(synth.get_data(cfg).train_dl))

"""Learner.validate over a validation set with repeated images, grouped (cfg group_val_by_image: each distinct image once per batch +
img_idx, the shared-image eval plan) against ungrouped (one image per query): the same ids, each once, and the same losses.

The CSV lists the rows of an image next to each other, so the grouped order equals the dataset order and both loaders cut the SAME
batches: the classification loss is normalised by the positives of the whole batch (loss.py:43-143), so batches of another
composition would average to another number whatever the network does.  pred_boxes are not compared here: an arg-max over the
anchors may flip on a rounding-level tie; the network-level comparison is tests/test_gpu_shared_net.py.

(The file is named to be collected behind test_gpu_streamk.py: the DevicePrefetchers made here take streams from torch's round-robin
pool, and that file's refusal test expects the next pool stream to be one nobody registered stream-K scratch for.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_validate_grouped_equals_ungrouped(tmp_path, gold):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import PIL.Image
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, evaluator, loss, mdl
    from zsgnet_pytorch_amd import dat_loader as D
    from zsgnet_pytorch_amd.trainer import Learner
    g = gold("g13_dataset")
    for k in "abc":
        PIL.Image.fromarray(g["png_" + k]).save(tmp_path / f"{k}.png")
    rows = list(zip(g["csv_img"], g["csv_bbox"], g["csv_query"]))
    names = sorted({str(r[0]) for r in rows})
    with open(tmp_path / "d.csv", "w") as f:
        f.write("img_id,bbox,query\n")
        for n in range(15):
            _, b, q = rows[n % len(rows)]
            f.write(f'{names[n // 5]},"{[float(v) + n % 3 for v in b]}","{q}"\n')
    np.savez(tmp_path / "vec.npz", words=g["words"], vectors=g["table"])
    kw = {"resize_img": [96, 64], "word_vectors": str(tmp_path / "vec.npz"), "ds_to_use": "refclef", "bs": 2, "bsv": 4, "nw": 0, "nwv": 0,
          "resnet_arch": "resnet18", "synthetic": False, "tmp_path": str(tmp_path / "run"),
          "ds_info.refclef.img_dir": str(tmp_path), "ds_info.refclef.trn_csv_file": str(tmp_path / "d.csv"),
          "ds_info.refclef.val_csv_file": str(tmp_path / "d.csv"), "ds_info.refclef.test_csv_file": str(tmp_path / "d.csv")}
    cfg0 = config.get_cfg(**kw)
    net = mdl.get_default_net(9, cfg0)
    net.load_state_dict(O.seeded_state_dict("resnet18", 2))
    net.to("cuda")
    net.lstm_state = "zeros"                       # (the reference draws the initial state per forward: the two passes must share it)
    r, s = config.ratios_scales(cfg0)
    lf, ev = loss.get_default_loss(r, s, cfg0), evaluator.get_default_eval(r, s, cfg0)
    res, ids, seen_idx = {}, {}, {}
    for grouped in (False, True):
        cfg = cfg0.clone()
        cfg["group_val_by_image"] = grouped
        data = D.get_data(cfg)
        assert isinstance(data.valid_dl, D.DevicePrefetcher)
        shapes = [(int(b["img"].shape[0]), int(b["qlens"].shape[0]), "img_idx" in b) for b in data.valid_dl]
        seen_idx[grouped] = shapes
        learn = Learner(f"g{int(grouped)}", data, net, lf, cfg, ev, None)
        res[grouped], preds = learn.validate(with_predictions=True)
        ids[grouped] = [int(p["id"]) for p in preds]
        assert all(np.isfinite(p["pred_scores"]) and len(p["pred_boxes"]) == 4 for p in preds)
    # the prefetcher uploads img_idx and resizes only the distinct images
    assert seen_idx[False] == [(4, 4, False), (4, 4, False), (4, 4, False), (3, 3, False)]
    assert seen_idx[True] == [(1, 4, True), (2, 4, True), (2, 4, True), (1, 3, True)]
    assert sorted(ids[True]) == list(range(15)) == sorted(ids[False])
    print("validate ungrouped", res[False])
    print("validate grouped  ", res[True])
    for k in lf.loss_keys:
        np.testing.assert_allclose(res[True][k], res[False][k], rtol=2e-4, err_msg=k)

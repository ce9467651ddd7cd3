"""Synthetic batches with the reference's batch contract (dat_loader.py:136-144, collater :187-196): every field a
float tensor — img [B,3,H,W] in [0,1), qvec [B,T,300], qlens [B], annot [B,4] y1x1y2x2 in [-1,1], idxs [B],
img_size [B,2] (h, w).  Distributions: SURVEY.md §8(d).  The CSV/PIL/spaCy loader itself is out of scope (§8 'next' N2)."""
from typing import Dict, Iterator

import torch


def synthetic_batch(B: int, H: int = 300, W: int = 300, T: int = 20, seed: int = 1234, tmax: int = 20, emb: int = 300) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g)
    qvec = torch.randn(B, T, emb, generator=g) * 0.35
    qlens = torch.randint(1, tmax + 1, (B,), generator=g).float()
    qlens[0] = float(tmax)
    c = torch.rand(B, 2, generator=g) * 1.2 - 0.6
    s = torch.rand(B, 2, generator=g) * 0.8 + 0.1
    annot = torch.cat([c - s / 2, c + s / 2], dim=1).clamp(-1, 1)
    return dict(img=img, qvec=qvec, qlens=qlens, annot=annot, idxs=torch.arange(B).float(),
                img_size=torch.tensor([[360.0, 480.0]]).repeat(B, 1))


def synthetic_shared_batch(Bi: int, Q: int, H: int = 300, W: int = 300, T: int = 20, seed: int = 1234, tmax: int = 20, emb: int = 300) -> Dict[str, torch.Tensor]:
    """A batch of Q queries over Bi <= Q distinct images (ZSGNet.forward's `img_idx` contract): `img` [Bi,3,H,W], the per-query fields
    of synthetic_batch with leading dimension Q, and `img_idx` [Q] int64 — shuffled, every image used at least once.  The per-query
    fields are exactly synthetic_batch(Q, ...)'s for the same seed; its Q images are not used."""
    if not 1 <= Bi <= Q:
        raise ValueError(f"synthetic_shared_batch: {Bi} images for {Q} queries")
    bt = synthetic_batch(Q, 8, 8, T, seed, tmax, emb)
    g = torch.Generator().manual_seed(seed + 7919)
    bt["img"] = torch.rand(Bi, 3, H, W, generator=g)
    idx = torch.cat([torch.arange(Bi), torch.randint(0, Bi, (Q - Bi,), generator=g)])
    bt["img_idx"] = idx[torch.randperm(Q, generator=g)].long()
    return bt


def expand_shared(bt: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the one-image-per-query batch a shared batch stands for: img[img_idx], no `img_idx`"""
    out = {k: v for k, v in bt.items() if k != "img_idx"}
    out["img"] = bt["img"].index_select(0, bt["img_idx"].long())
    return out


class SyntheticLoader:
    """Iterable with len(): `steps` batches per epoch, deterministic per (seed, rank, step); a pool of `pool` distinct
    batches is generated once on the host and kept on the device (generating 16 x 3 x 300 x 300 uniform numbers on the CPU
    every step costs as much as the GPU training step itself), then cycled with fresh row ids."""

    def __init__(self, cfg, bs: int, steps: int, seed: int = 1234, rank: int = 0, device="cuda", pool: int = 8, group_k: int = 0):
        """group_k > 0 (the training loader under cfg group_trn_by_image): batches of bs queries over bs // group_k image slots with
        `img_idx`, group_k queries per slot in shuffled order — what dat_loader's grouped training loader makes."""
        self.cfg, self.bs, self.steps, self.seed, self.rank, self.device = cfg, bs, steps, seed, rank, device
        if group_k and (bs < group_k or bs % group_k):
            raise ValueError(f"grouped training loader: bs={bs} must be a positive multiple of trn_queries_per_image={group_k}")
        self.group_k = int(group_k)
        self.epoch = 0
        self.pool, self._cache = pool, {}

    def __len__(self):
        return self.steps

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        H, W = self.cfg["resize_img"]
        dev = torch.device(self.device if torch.cuda.is_available() else "cpu")
        for i in range(self.steps):
            k = i % self.pool
            if k not in self._cache:
                sd = self.seed + 1000003 * self.rank + k
                if self.group_k:
                    Bi = self.bs // self.group_k
                    bt = synthetic_shared_batch(Bi, self.bs, H, W, seed=sd, emb=self.cfg["emb_dim"])
                    g = torch.Generator().manual_seed(sd + 104729)
                    bt["img_idx"] = torch.arange(Bi).repeat_interleave(self.group_k)[torch.randperm(self.bs, generator=g)]       # equal groups
                else:
                    bt = synthetic_batch(self.bs, H, W, seed=sd, emb=self.cfg["emb_dim"])
                self._cache[k] ={n: v.to(dev) for n, v in bt.items()}
            bt = dict(self._cache[k])
            bt["idxs"] = bt["idxs"] + float((self.rank * self.steps + i) * self.bs)      # dataset row ids (dat_loader.py:140), unique per sample
            yield bt
        self.epoch += 1


class DataWrap:
    """utils.py:116-120"""

    def __init__(self, train_dl, valid_dl, test_dl=None, path="./tmp"):
        self.train_dl, self.valid_dl, self.test_dl, self.path = train_dl, valid_dl, test_dl, path


def get_data(cfg, rank: int = 0) -> DataWrap:
    """dat_loader.get_data counterpart for synthetic runs (per-rank batch = cfg.bs, dat_loader.py:212-215)."""
    steps = int(cfg["steps_per_epoch"])
    gk = int(cfg["trn_queries_per_image"]) if ("group_trn_by_image" in cfg and cfg["group_trn_by_image"]) else 0
    return DataWrap(SyntheticLoader(cfg, cfg["bs"], steps, 1234, rank, group_k=gk),SyntheticLoader(cfg, cfg["bsv"], max(1, steps // 5), 4321, rank),
                    {"synthetic_test": SyntheticLoader(cfg, cfg["bsv"], max(1, steps // 5), 9999, rank)}, cfg["tmp_path"])

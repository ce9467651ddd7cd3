"""Reference of the weight EMA tests: the fp64 recurrence e <- e + w (p - e) over recorded fp32 snapshots, the decay schedule, and the error
bound of the fp32 kernels against it.

Bound of ONE fp32 update ema <- fmaf(w, p - ema, ema), elementwise: 2**-22 * max(|e|, |p|).  Two roundings: fl(p - e) is off by at most
2**-23 * max(|e|, |p|) (half an ulp of a difference of magnitude <= 2 max), scaled by w <= 1; the final rounding of a result of magnitude
<= max(|e|, |p|) adds at most 2**-24 * max.  The total is below 1.5 * 2**-23 * max; the bound is the next power of two.  It holds whether
or not the multiply-add is fused (an unfused product adds one more rounding of w * d, at most 2**-24 * 2 max * w, still inside).
A k-update trajectory gets k times the bound with the maximum magnitude taken over the whole trajectory (every step's own error is
bounded by the one-step bound at that step's magnitudes, and an error carried into a step leaves it scaled by 1 - w <= 1).
Every comparison covers all elements."""
import numpy as np
import torch

UNIT = 2.0 ** -22


def decay_at(decay: float, warmup: bool, n: int) -> float:
    """decay of the update after n earlier ones"""
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def weight(decay: float, warmup: bool, n: int) -> float:
    """w of the update after n earlier ones, as the fp32 value the kernels receive: the first is a copy"""
    return 1.0 if n == 0 else float(np.float32(1.0 - decay_at(decay, warmup, n)))


def step64(e: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    """one update in fp64 (w == 1 is a copy by definition)"""
    e, p = e.double(), p.double()
    return p.clone() if w == 1.0 else e + w * (p - e)


def bound1(e: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """the bound of one fp32 update from e with p"""
    return UNIT * torch.maximum(e.double().abs(), p.double().abs())


def trajectory(snaps, decay: float, warmup: bool = False, n0: int = 0, e0=None):
    """(fp64 average, elementwise bound) after one update per snapshot (fp32 tensors, CPU), starting from e0 after n0 earlier updates"""
    e = None if e0 is None else e0.double()
    mag = torch.zeros_like(snaps[0], dtype=torch.float64) if e is None else e.abs()
    k = 0
    for i, p in enumerate(snaps):
        w = weight(decay, warmup, n0 + i)
        e = step64(p if e is None else e, p, w)
        mag = torch.maximum(mag, torch.maximum(e.abs(), p.double().abs()))
        k += 0 if w == 1.0 else 1            # (a copy is exact)
    return e, max(k, 1) * UNIT * mag


def assert_within(got: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str = ""):
    """|got - ref| <= bound on EVERY element (prints the worst ratio first)"""
    err = (got.double().cpu() - ref64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / bound {ratio:.3f} over {err.numel()} elements")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound (worst ratio {ratio:.3f})"

"""zsg_conv_wgrad_bf16 / zsg_conv_wgrad_bf16_supported (csrc/wgrad_bf16.hip) at the kernel level, through the C ABI.

Bounds, none of them taken from what the code gives:
  * integer data in [-8, 8]: every product is at most 64 and every partial sum stays below 2^24 (rows <= 722 here, so
    |sum| <= 64 * 722 + 8), integers of that size are exact in bf16 (|v| <= 8) and fp32: the result is exact in ANY summation order,
    slab reduction included — zero tolerance against int64 arithmetic (tests/wgrad_bf16_ref.py);
  * standard-normal data: fp64 weight gradient of the HOST-rounded bf16 operands; per element
    |dw - ref| <= (rows + 4) * 2^-23 * (S + |dw_prev|), S the same sum over absolute values, rows = the GEMM's K (pixel rows of all
    segments) — the worst case of any fp32 accumulation order with a relative error of at most 2^-23 per operation.  K is small on
    purpose: at 9 and 722 rows a truncating conversion breaks this bound on nearly every element.
Every src / dy buffer has guard rows of NaN in front and behind; dw is pre-filled with NaN (or a sentinel where a window is tested), so
an element that was not written, a read of dw with accumulate == 0 or of memory outside the operands shows."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_bf16_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# 0 = the library heuristic, else (BM, BN, splits); splits == 1 runs with ws = NULL
HINTS = (0, (64, 64, 1), (128, 64, 3), (64, 128, 2), (128, 128, 5))
GUARD = 4096          # NaN elements in front of and behind every operand buffer
SENTINEL = 7.0

# name -> (levels [(H, W)], B, C, N, k, stride, pad, dil, extras)
CASES = {
    "tiny_rows": ([(3, 3)], 1, 64, 64, 1, 1, 0, 1, {}),
    "rows_tail": ([(19, 19)], 2, 64, 64, 1, 1, 0, 1, {}),
    "pad3x3": ([(20, 17)], 2, 64, 128, 3, 1, 1, 1, {}),
    "stride2": ([(21, 21)], 2, 128, 128, 3, 2, 1, 1, {}),
    "strided_1x1": ([(9, 11)], 3, 256, 64, 1, 2, 0, 1, {}),
    "dil6": ([(12, 12)], 1, 64, 96, 3, 1, 6, 6, {}),
    "c36": ([(7, 9)], 2, 36, 72, 3, 1, 1, 1, {}),
    "c40": ([(7, 9)], 2, 40, 72, 3, 1, 1, 1, {}),
    "conv0_516": ([(10, 10)], 1, 256, 256, 3, 1, 1, 1, dict(wC=516, wc0=0)),
    "window_wc0": ([(8, 8)], 2, 64, 64, 1, 1, 0, 1, dict(wC=132, wc0=64)),
    "n45": ([(10, 10)], 2, 256, 45, 3, 1, 1, 1, dict(out_ld=48)),
    "shared_head": ([(10, 10), (5, 5), (3, 3)], 2, 256, 256, 3, 1, 1, 1, {}),
    "accumulate": ([(19, 19)], 2, 64, 64, 1, 1, 0, 1, dict(accumulate=True)),
    "overwrite": ([(20, 17)], 2, 64, 128, 3, 1, 1, 1, {}),        # accumulate = 0 on a NaN-filled dw (what every case here does; named)
}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, ops
    return _lib, ops


@functools.lru_cache(maxsize=None)
def make_case(name, kind):
    """operands (fp32, CPU) and the reference of one case, computed once and shared by the tests (never modified)"""
    levels, B, Cc, N, k, s, p, d, ex = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) * 2 + (kind == "int"))

    def draw(*shape):
        if kind == "int":
            return torch.randint(-8, 9, shape, generator=g).float()
        return torch.randn(*shape, generator=g)
    srcs = [draw(B, H, W, Cc) for (H, W) in levels]
    outs_hw = [(R.conv_out(H, k, s, p, d), R.conv_out(W, k, s, p, d)) for (H, W) in levels]
    dys = [draw(B, Ho, Wo, N) for (Ho, Wo) in outs_hw]
    rows = sum(B * Ho * Wo for (Ho, Wo) in outs_hw)
    prev = draw(N, k, k, Cc) if ex.get("accumulate") else None
    if kind == "int":
        ref = R.wgrad_ref_levels([x.to(torch.int64) for x in srcs], [y.to(torch.int64) for y in dys], k, s, p, d)
        if prev is not None:
            ref = ref + prev.to(torch.int64)
        assert int(ref.abs().max()) < 2 ** 24 and rows <= 722
        ref, bound = ref.float(), None
    else:
        xs, ys = [R.bf16_round(x) for x in srcs], [R.bf16_round(y) for y in dys]
        ref = R.wgrad_ref_levels(xs, ys, k, s, p, d)
        S = R.wgrad_ref_levels([x.abs() for x in xs], [y.abs() for y in ys], k, s, p, d)
        if prev is not None:
            ref, S = ref + prev.double(), S + prev.double().abs()
        bound = (rows + 4) * 2.0 ** -23 * S
    return dict(srcs=srcs, dys=dys, outs_hw=outs_hw, rows=rows, prev=prev, ref=ref, bound=bound)


def guarded(parts):
    """one device buffer: NaN guard, the parts back to back, NaN guard; returns (buffer, element offset of each part)"""
    offs, o = [], GUARD
    for t in parts:
        offs.append(o)
        o += t.numel()
    buf = torch.full((o + GUARD,), float("nan"))
    for t, of in zip(parts, offs):
        buf[of:of + t.numel()] = t.reshape(-1)
    return buf.cuda(), offs


def launch(Z, name, kind, hint, small_ws=False):
    """run one case; returns (dw window [N, k, k, C] on the CPU, the whole dw [N, k, k, wC], rc)"""
    L, ops = Z
    levels, B, Cc, N, k, s, p, d, ex = CASES[name]
    cs = make_case(name, kind)
    wC, wc0, old = ex.get("wC", Cc), ex.get("wc0", 0), ex.get("out_ld", N)
    src_buf, s_off = guarded(cs["srcs"])
    dy_parts = []
    for y in cs["dys"]:
        yp = torch.full(y.shape[:3] + (old,), float("nan"))       # the row padding N..out_ld-1 is NaN: it must never enter a sum
        yp[..., :N] = y
        dy_parts.append(yp)
    dy_buf, d_off = guarded(dy_parts)
    lv_s = [ops.Level(o, H, W, H * W * Cc) for o, (H, W) in zip(s_off, levels)]
    lv_o = [ops.Level(o, Ho, Wo, Ho * Wo * old) for o, (Ho, Wo) in zip(d_off, cs["outs_hw"])]
    windowed = wC != Cc
    dw = torch.full((N, k, k, wC), SENTINEL if windowed else float("nan"))
    acc = 1 if ex.get("accumulate") else 0
    if acc:
        dw[..., wc0:wc0 + Cc] = cs["prev"]
    dw = dw.cuda()
    th = 0 if hint == 0 else ops.tile_hint(*hint)
    desc = ops.fwd_desc(ops.TView(src_buf, B, Cc, Cc, lv_s), ops.TView(dy_buf, B, N, old, lv_o), Cc, N, k, s, p, d, wC=wC, wc0=wc0, tile_hint=th)
    ok = int(L.lib.zsg_conv_wgrad_bf16_supported(C.byref(desc)))
    if hint != 0 and hint[2] == 1:
        ws, ws_bytes = None, 0
    else:
        ws_bytes = int(L.lib.zsg_conv_wgrad_workspace_bytes(C.byref(desc)))
        if small_ws:
            ws_bytes = 2 * N * k * k * Cc * 4 - 4
        ws = torch.full((ws_bytes // 4 + 1,), float("nan"), device="cuda")
    rc = L.lib.zsg_conv_wgrad_bf16(C.byref(desc), src_buf.data_ptr(), dy_buf.data_ptr(), dw.data_ptr(), acc, ws.data_ptr() if ws is not None else None,
                                   ws_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    assert ok == (1 if rc in (0, -2) else 0), f"_supported says {ok}, the entry returned {rc}"
    full = dw.cpu()
    return full[..., wc0:wc0 + Cc].contiguous(), full, rc


def check_outside_window(name, full):
    _, _, Cc, _, _, _, _, _, ex = CASES[name]
    wC, wc0 = ex.get("wC", Cc), ex.get("wc0", 0)
    if wC != Cc:
        keep = torch.ones(wC, dtype=torch.bool)
        keep[wc0:wc0 + Cc] = False
        assert bool((full[..., keep] == SENTINEL).all()), f"{name}: dw written outside the channel window"


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_is_exact(Z, name):
    cs = make_case(name, "int")
    for hint in HINTS:
        got, full, rc = launch(Z, name, "int", hint)
        assert rc == 0, Z[0].lib.zsg_last_error().decode()
        ref = cs["ref"]
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), \
            f"{name} hint {hint}: {int((got != ref).sum())} of {ref.numel()} elements differ, max |diff| {float((got - ref).abs().max())}"
        check_outside_window(name, full)


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_data_within_the_fp32_accumulation_bound(Z, name):
    cs = make_case(name, "rand")
    worst = 0.0
    for hint in HINTS:
        got, full, rc = launch(Z, name, "rand", hint)
        assert rc == 0, Z[0].lib.zsg_last_error().decode()
        assert not torch.isnan(got).any(), f"{name} hint {hint}: unwritten or NaN-polluted gradient elements"
        err = (got.double() - cs["ref"]).abs()
        frac = float((err / cs["bound"].clamp(min=1e-300)).max())
        worst = max(worst, frac)
        assert bool((err <= cs["bound"]).all()), f"{name} hint {hint}: max error / bound = {frac:.3f} (rows = {cs['rows']})"
        check_outside_window(name, full)
    print(f"bf16 wgrad {name}: largest |dw - ref| / bound over all tile hints = {worst:.4f}")


def test_two_runs_write_identical_bits(Z):
    for name in ("shared_head", "rows_tail"):
        for hint in HINTS:
            a, _, rc = launch(Z, name, "rand", hint)
            b, _, _ = launch(Z, name, "rand", hint)
            assert rc == 0
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, hint)


def test_workspace_too_small_is_minus_two(Z):
    got, full, rc = launch(Z, "rows_tail", "rand", (64, 64, 4), small_ws=True)
    assert rc == -2 and "workspace" in Z[0].lib.zsg_last_error().decode()
    assert bool(torch.isnan(full).all()), "a refused call must launch nothing"
    got, full, rc = launch(Z, "rows_tail", "rand", (64, 64, 2), small_ws=True)      # two slabs fit... one element short
    assert rc == -2


def test_refusals_and_supported_agree(Z):
    L, ops = Z
    x = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    g = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    dw = torch.full((64 * 64,), SENTINEL, device="cuda")
    ws = torch.zeros(64 * 64 * 64, device="cuda")
    lv = [ops.Level(0, 8, 8, 8 * 8 * 64)]

    def desc(out_ld=64, **kw):
        d = ops.fwd_desc(ops.TView(x, 2, 64, 64, lv), ops.TView(g, 2, 64, out_ld, lv), 64, 64, 1, 1, 0, 1, wC=64)
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d
    wide_s, wide_o = desc(), desc()
    wide_s.seg[0].src_bstride = 1 << 23
    wide_o.seg[0].out_bstride = 1 << 23
    bad = {
        "merge_x": desc(merge_x=1),
        "out_ld % 4": desc(out_ld=46, N=46),
        "src image stride 2^23": wide_s,
        "dy image stride 2^23": wide_o,
        "bit 24 (8-wave)": desc(tile_hint=ops.tile_hint(128, 128, 2, 1)),
        "bit 25 (32-pixel K tiles)": desc(tile_hint=ops.tile_hint(64, 64, 2, 0, 1)),
        "bit 26": desc(tile_hint=ops.tile_hint(64, 64, 2) | (1 << 26)),
        "bit 27": desc(tile_hint=ops.tile_hint(64, 64, 2) | (1 << 27)),
        "BN 255": desc(tile_hint=ops.tile_hint(64, 255, 2)),
    }
    for what, d in bad.items():
        assert L.lib.zsg_conv_wgrad_bf16_supported(C.byref(d)) == 0, what
        rc = L.lib.zsg_conv_wgrad_bf16(C.byref(d), x.data_ptr(), g.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, L.stream_ptr())
        msg = L.lib.zsg_last_error().decode()
        assert rc == -1 and "conv_wgrad_bf16" in msg and len(msg) > 25, (what, rc, msg)
    torch.cuda.synchronize()
    assert float(dw.min()) == SENTINEL and float(dw.max()) == SENTINEL, "a refused call must launch nothing"
    good = desc()
    assert L.lib.zsg_conv_wgrad_bf16_supported(C.byref(good)) == 1
    assert L.lib.zsg_conv_wgrad_bf16(C.byref(good), None, g.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, L.stream_ptr()) == -1
    assert L.lib.zsg_conv_wgrad_bf16(C.byref(good), x.data_ptr(), g.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0.0

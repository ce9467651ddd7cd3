"""zsg_conv_igemm_bf16_io / zsg_conv_igemm_bf16_io_supported (csrc/igemm_bf16.hip) at the kernel level: the bf16 convolution with each of
src / out / add_src stored as fp32 or bf16 (io_flags SRC_BF16 = 1, OUT_BF16 = 2, ADD_BF16 = 4).

References and bounds, none taken from what the code gives (the first two are test_gpu_conv_bf16.py's):
  * integer data in [-8, 8] (exact in bf16): every product and partial sum stays below 2^24, so the fp32 value in front of the store is
    exact in any summation order; expected = int64 convolution (+ bias + add, ReLU), and for a bf16 output that value through
    .float().to(torch.bfloat16) — zero tolerance.  Sums reach ~1e5 (17 significant bits), so the store's rounding to 8 bits, ties
    included (integers are dense among the tie points), is exercised;
  * standard-normal data: fp64 convolution of the HOST-rounded bf16 operands (add_src host-rounded too where it is stored as bf16);
    E = (K + 4) * 2^-23 * (S + |bias| + |add|) bounds any fp32 accumulation order; an fp32 output must lie within E, a bf16 output within
    E + 2^-8 * (|ref| + E): half the spacing of bf16 at the magnitude of the value that is rounded (spacing <= 2^-7 * |v|) — derived;
  * untouched memory: every output buffer is filled with a NaN bit pattern in front of the launch; row padding (out_ld > N) and the
    guard elements behind the last row must still hold it afterwards.
The tile hints 0, 64x64, 128x64, 128x128 run on the first five cases."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_conv_bf16 import conv_out, conv_ref, pack_jobs  # noqa: E402  (the independent references of the fp32-in-memory kernel's test)

SRC, OUT, ADD = 1, 2, 4
HINTS = (0, (64, 64), (128, 64), (128, 128))
GUARD = 64
BF = torch.bfloat16

# name -> (levels [(H, W)], B, C, N, k, stride, pad, extras); extras: flags (default SRC | OUT), bias, relu, add, alias, out_ld
CASES = {
    "rows_tail": ([(19, 19)], 2, 64, 64, 1, 1, 0, dict(out_ld=72)),
    "c36": ([(7, 9)], 2, 36, 72, 3, 1, 1, {}),                         # src_ld = 36: 8-byte rows, a half-group tail
    "c40": ([(7, 9)], 2, 40, 72, 3, 1, 1, {}),
    "stride2": ([(21, 21)], 2, 128, 128, 3, 2, 1, {}),
    "n45": ([(10, 10)], 2, 256, 45, 3, 1, 1, dict(bias=True)),         # out_ld = 45: 2-byte stores at odd element offsets
    "n45_f32out": ([(10, 10)], 2, 256, 45, 3, 1, 1, dict(bias=True, flags=SRC)),      # the head's last convolution
    "residual": ([(16, 16)], 2, 64, 256, 1, 1, 0, dict(add=True, relu=True, flags=SRC | OUT | ADD)),
    "alias": ([(16, 16)], 2, 64, 256, 1, 1, 0, dict(add=True, relu=True, alias=True, flags=SRC | OUT | ADD)),
    "shared_head": ([(10, 10), (5, 5), (3, 3)], 2, 256, 256, 3, 1, 1, dict(bias=True, relu=True)),
    "y_fp32": ([(10, 10), (5, 5), (3, 3)], 2, 256, 256, 3, 1, 1, dict(flags=SRC)),          # conv0's feature GEMM of the shared plan
    "conv0_lmap": ([(10, 10)], 2, 256, 256, 3, 1, 1, dict(bias=True, relu=True, add=True)),   # bf16 in / out, the fp32 language map added
    "f32_in": ([(9, 11)], 2, 4, 64, 3, 1, 1, dict(relu=True, flags=OUT)),                   # an fp32 image into a bf16 activation
}
FIRST_FIVE = ("rows_tail", "c36", "c40", "stride2", "n45")


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, ops
    return _lib, ops


def flags_of(name):
    return CASES[name][7].get("flags", SRC | OUT)


@functools.lru_cache(maxsize=None)
def make_case(name, kind, flags=None):
    """operands (fp32 values on the CPU; for `rand` already host-rounded where they are stored as bf16) and the reference, once"""
    levels, B, Cc, N, k, s, p, ex = CASES[name]
    flags = flags_of(name) if flags is None else flags
    g = torch.Generator().manual_seed(100 + sorted(CASES).index(name) * 2 + (kind == "int"))

    def draw(*shape):
        if kind == "int":
            return torch.randint(-8, 9, shape, generator=g).float()
        return torch.randn(*shape, generator=g)
    w = draw(N, k, k, Cc)
    srcs = [draw(B, H, W, Cc) for (H, W) in levels]
    if flags & SRC:
        srcs = [x.to(BF).float() for x in srcs]
    outs_hw = [(conv_out(H, k, s, p, 1), conv_out(W, k, s, p, 1)) for (H, W) in levels]
    bias = draw(N) if ex.get("bias") else None
    adds = [draw(B, Ho, Wo, N) for (Ho, Wo) in outs_hw] if ex.get("add") else None
    if adds is not None and flags & ADD:
        adds = [a.to(BF).float() for a in adds]
    refs, bounds = [], []
    for i, (x, (Ho, Wo)) in enumerate(zip(srcs, outs_hw)):
        if kind == "int":
            r = conv_ref(x.to(torch.int64), w.to(torch.int64), k, s, p, 1, Ho, Wo)
            if bias is not None:
                r = r + bias.to(torch.int64)
            if adds is not None:
                r = r + adds[i].to(torch.int64)
            if ex.get("relu"):
                r = r.clamp(min=0)
            assert int(r.abs().max()) < 2 ** 24
            r = r.float()
            refs.append(r.to(BF).float() if flags & OUT else r)
            bounds.append(None)
        else:
            xb, wb = x.to(BF).double(), w.to(BF).double()
            r = conv_ref(xb, wb, k, s, p, 1, Ho, Wo)
            S = conv_ref(xb.abs(), wb.abs(), k, s, p, 1, Ho, Wo)
            if bias is not None:
                r, S = r + bias.double(), S + bias.double().abs()
            if adds is not None:
                r, S = r + adds[i].double(), S + adds[i].double().abs()
            if ex.get("relu"):
                r = r.clamp(min=0)
            E = (k * k * Cc + 4) * 2.0 ** -23 * S
            refs.append(r)
            bounds.append(E + 2.0 ** -8 * (r.abs() + E) if flags & OUT else E)
    return dict(w=w, srcs=srcs, outs_hw=outs_hw, bias=bias, adds=adds, refs=refs, bounds=bounds, flags=flags)


def poisoned(n, b16):
    """n elements of a NaN bit pattern (0x7FC0 / 0x7FC00000) + the guard"""
    if b16:
        return torch.full((n + GUARD,), 0x7FC0, dtype=torch.int16, device="cuda").view(BF)
    return torch.full((n + GUARD,), float("nan"), device="cuda")


def launch(Z, name, kind, hint, flags=None, src_f32_of=None):
    """run one case; returns (per-level outputs [B, Ho, Wo, N] as fp32 on the CPU, rc, the whole output buffer on the CPU).
    src_f32_of: feed THESE fp32 sources (flags without SRC) instead of the case's."""
    L, ops = Z
    levels, B, Cc, N, k, s, p, ex = CASES[name]
    cs = make_case(name, kind, flags)
    flags = cs["flags"]
    out_ld = ex.get("out_ld", N)
    (wp,) = pack_jobs(L, [(cs["w"].cuda(), N, k * k, Cc, 0, Cc)])
    srcs = src_f32_of if src_f32_of is not None else cs["srcs"]
    src_flat = torch.cat([x.reshape(-1) for x in srcs]).cuda()
    if flags & SRC:
        src_flat = src_flat.to(BF)
    lv_s, lv_o, so, oo = [], [], 0, 0
    for (H, W), (Ho, Wo) in zip(levels, cs["outs_hw"]):
        lv_s.append(ops.Level(so, H, W, H * W * Cc))
        lv_o.append(ops.Level(oo, Ho, Wo, Ho * Wo * out_ld))
        so += B * H * W * Cc
        oo += B * Ho * Wo * out_ld
    out = poisoned(oo, bool(flags & OUT))
    add = None
    if cs["adds"] is not None:
        assert out_ld == N
        add = torch.cat([a.reshape(-1) for a in cs["adds"]]).cuda()
        add = add.to(BF) if flags & ADD else add
        if ex.get("alias"):
            assert bool(flags & ADD) == bool(flags & OUT)
            out[:oo].copy_(add)
            add = out
    bias = cs["bias"].cuda() if cs["bias"] is not None else None
    th = 0 if hint == 0 else ops.tile_hint(hint[0], hint[1], 1)
    desc = ops.fwd_desc(ops.TView(src_flat, B, Cc, Cc, lv_s), ops.TView(out, B, N, out_ld, lv_o), Cc, N, k, s, p, 1, wC=Cc,
                        relu=bool(ex.get("relu")), tile_hint=th)
    ok = int(L.lib.zsg_conv_igemm_bf16_io_supported(C.byref(desc), flags))
    rc = L.lib.zsg_conv_igemm_bf16_io(C.byref(desc), src_flat.data_ptr(), wp.data_ptr(), out.data_ptr(), bias.data_ptr() if bias is not None else None,
                                      add.data_ptr() if add is not None else None, flags, L.stream_ptr())
    torch.cuda.synchronize()
    assert ok == (1 if rc == 0 else 0), f"_io_supported says {ok}, the entry returned {rc}: {L.lib.zsg_last_error().decode()}"
    oc = out.cpu()
    res, o = [], 0
    for (Ho, Wo) in cs["outs_hw"]:
        blk = oc[o:o + B * Ho * Wo * out_ld].view(B, Ho, Wo, out_ld)
        res.append(blk[..., :N].float())
        assert bool(torch.isnan(blk[..., N:]).all()), f"{name}: row padding was written"
        o += B * Ho * Wo * out_ld
    assert bool(torch.isnan(oc[oo:]).all()), f"{name}: elements behind the last row were written"
    return res, rc, oc


def check_int(Z, name, hint):
    cs = make_case(name, "int")
    res, rc, _ = launch(Z, name, "int", hint)
    assert rc == 0, Z[0].lib.zsg_last_error().decode()
    for lvl, (got, ref) in enumerate(zip(res, cs["refs"])):
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), \
            f"{name} hint {hint} level {lvl}: {int((got != ref).sum())} of {ref.numel()} elements differ, max |diff| {float((got - ref).abs().max())}"
    return max(float(r.abs().max()) for r in cs["refs"])


def check_rand(Z, name, hint):
    cs = make_case(name, "rand")
    res, rc, _ = launch(Z, name, "rand", hint)
    assert rc == 0, Z[0].lib.zsg_last_error().decode()
    worst = 0.0
    for lvl, (got, ref, bound) in enumerate(zip(res, cs["refs"], cs["bounds"])):
        assert not torch.isnan(got).any(), f"{name} hint {hint}: unwritten output elements"
        err = (got.double() - ref).abs()
        frac = float((err / bound.clamp(min=1e-300)).max())
        worst = max(worst, frac)
        assert bool((err <= bound).all()), f"{name} hint {hint} level {lvl}: max error / bound = {frac:.3f}"
    return worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_is_exact(Z, name):
    top = 0.0
    for hint in (HINTS if name in FIRST_FIVE else (0,)):
        top = max(top, check_int(Z, name, hint))
    print(f"bf16_io conv {name} (flags {flags_of(name)}): integer data exact, max |ref| {top:.0f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_data_within_the_derived_bound(Z, name):
    worst = 0.0
    for hint in (HINTS if name in FIRST_FIVE else (0,)):
        worst = max(worst, check_rand(Z, name, hint))
    print(f"bf16_io conv {name} (flags {flags_of(name)}): largest |out - ref| / bound = {worst:.4f}")


def test_integer_sums_exercise_the_store_rounding():
    """the integer references are not all bf16-representable before the store: the rounding (and exact ties) really happens"""
    levels, B, Cc, N, k, s, p, ex = CASES["stride2"]
    cs = make_case("stride2", "int")
    x, w = cs["srcs"][0].to(torch.int64), cs["w"].to(torch.int64)
    raw = conv_ref(x, w, k, s, p, 1, *cs["outs_hw"][0]).float()
    rounded = raw.to(BF).float()
    assert int((raw != rounded).sum()) > raw.numel() // 4
    r = raw.view(torch.int32)
    ties = ((r & 0xFFFF) == 0x8000)                      # exactly half-way between two bf16 values
    assert int(ties.sum()) > 0, "no tie among the integer sums of this case"
    assert torch.equal(cs["refs"][0], rounded)


@pytest.mark.parametrize("flags", range(8))
def test_every_flag_word_on_the_residual_case(Z, flags):
    """all eight storage combinations on 1x1 + add + ReLU (integer data, exact)"""
    cs = make_case("residual", "int", flags)
    res, rc, _ = launch(Z, "residual", "int", 0, flags)
    assert rc == 0, Z[0].lib.zsg_last_error().decode()
    assert torch.equal(res[0].view(torch.int32), cs["refs"][0].view(torch.int32))
    cs = make_case("residual", "rand", flags)
    res, rc, _ = launch(Z, "residual", "rand", (128, 128), flags)
    assert rc == 0 and bool(((res[0].double() - cs["refs"][0]).abs() <= cs["bounds"][0]).all())


@pytest.mark.parametrize("name", ("rows_tail", "c36", "shared_head"))
def test_bf16_source_writes_the_bits_of_the_converting_loader(Z, name):
    """src = x.to(bf16) with SRC_BF16 gives the operand bits the fp32 loader makes of x: flags = SRC and flags = 0 write the same fp32
    output, bit for bit; and two runs are identical"""
    levels, B, Cc, N, k, s, p, ex = CASES[name]
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(B, H, W, Cc, generator=g) for (H, W) in levels]                   # NOT bf16-representable
    for hint in (0, (128, 64)):
        _, rc0, a = launch(Z, name, "rand", hint, flags=0, src_f32_of=xs)
        _, rc1, b = launch(Z, name, "rand", hint, flags=SRC, src_f32_of=[x.to(BF).float() for x in xs])
        _, _, b2 = launch(Z, name, "rand", hint, flags=SRC, src_f32_of=[x.to(BF).float() for x in xs])
        assert rc0 == 0 and rc1 == 0
        n = a.numel() - GUARD
        pad = torch.isnan(a[:n])
        assert torch.equal(pad, torch.isnan(b[:n])) and int((~pad).sum()) > 0
        assert torch.equal(a[:n][~pad].view(torch.int32), b[:n][~pad].view(torch.int32)), f"{name} hint {hint}"
        assert torch.equal(b.view(torch.int32), b2.view(torch.int32))


def test_io0_is_the_existing_entry(Z):
    """io_flags = 0 writes what zsg_conv_igemm_bf16 writes"""
    L, ops = Z
    g = torch.Generator().manual_seed(11)
    B, H, W, Cc, N = 2, 9, 7, 64, 64
    x = torch.randn(B * H * W * Cc, generator=g).cuda()
    (wp,) = pack_jobs(L, [(torch.randn(N, 9, Cc, generator=g).cuda(), N, 9, Cc, 0, Cc)])
    lv = [ops.Level(0, H, W, H * W * Cc)]
    outs = []
    for io in (None, 0):
        out = torch.full((B * H * W * N,), float("nan"), device="cuda")
        d = ops.fwd_desc(ops.TView(x, B, Cc, Cc, lv), ops.TView(out, B, N, N, lv), Cc, N, 3, 1, 1, 1, wC=Cc, relu=True)
        if io is None:
            L.check(L.lib.zsg_conv_igemm_bf16(C.byref(d), x.data_ptr(), wp.data_ptr(), out.data_ptr(), None, None, L.stream_ptr()), "bf16")
        else:
            L.check(L.lib.zsg_conv_igemm_bf16_io(C.byref(d), x.data_ptr(), wp.data_ptr(), out.data_ptr(), None, None, 0, L.stream_ptr()), "io")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and not torch.isnan(outs[0]).any()


def test_refusals_and_supported_agree(Z):
    L, ops = Z
    x = torch.zeros(2 * 8 * 8 * 64, dtype=BF, device="cuda")
    o = torch.zeros(2 * 8 * 8 * 64, dtype=BF, device="cuda")
    wp = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    lv = [ops.Level(0, 8, 8, 8 * 8 * 64)]

    def desc(**kw):
        d = ops.fwd_desc(ops.TView(x, 2, 64, 64, lv), ops.TView(o, 2, 64, 64, lv), 64, 64, 1, 1, 0, 1, wC=64)
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d
    bad = {
        "merge_x": (desc(merge_x=1), 3),
        "split-K": (desc(tile_hint=ops.tile_hint(64, 64, 2)), 3),
        "stream-K": (desc(tile_hint=ops.tile_hint(64, 64, 1) | (1 << 28)), 3),
        "8-wave bit": (desc(tile_hint=ops.tile_hint(64, 64, 1, 1)), 3),
        "epi_flags": (desc(epi_flags=1), 3),
        "src_ld 34": (desc(C=32, src_ld=34), 3),
        "flag word": (desc(), 8),
    }
    o.fill_(3.0)
    for what, (d, io) in bad.items():
        assert L.lib.zsg_conv_igemm_bf16_io_supported(C.byref(d), io) == 0, what
        rc = L.lib.zsg_conv_igemm_bf16_io(C.byref(d), x.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, io, L.stream_ptr())
        msg = L.lib.zsg_last_error().decode()
        assert rc == -1 and "conv_igemm_bf16_io" in msg and len(msg) > 20, (what, rc, msg)
    # refusals the DESCRIPTOR cannot show: ADD_BF16 without add_src; a bf16 src that is not 8-byte aligned
    good = desc()
    assert L.lib.zsg_conv_igemm_bf16_io_supported(C.byref(good), SRC | OUT | ADD) == 1
    rc = L.lib.zsg_conv_igemm_bf16_io(C.byref(good), x.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, SRC | OUT | ADD, L.stream_ptr())
    assert rc == -1 and "ADD_BF16" in L.lib.zsg_last_error().decode()
    rc = L.lib.zsg_conv_igemm_bf16_io(C.byref(good), x.data_ptr() + 2, wp.data_ptr(), o.data_ptr(), None, None, SRC | OUT, L.stream_ptr())
    assert rc == -1 and "aligned" in L.lib.zsg_last_error().decode()
    torch.cuda.synchronize()
    assert float(o.float().min()) == 3.0 and float(o.float().max()) == 3.0, "a refused call must launch nothing"
    assert L.lib.zsg_conv_igemm_bf16_io(C.byref(good), x.data_ptr(), wp.data_ptr(), o.data_ptr(), None, None, SRC | OUT, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(o.float().abs().max()) == 0.0

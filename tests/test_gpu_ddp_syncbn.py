"""Synchronized BatchNorm across data-parallel ranks (dist.convert_sync_batchnorm): two ranks share ONE GPU over gloo (as
test_gpu_ddp_clip.py) and are compared with one process that runs the concatenated batch.  With ZSG_DETERMINISTIC=1:
- each rank's outputs equal the matching rows of the full-batch outputs, and both ranks' running statistics the full batch's;
- world x the reduced gradient equals the full-batch gradient (backward driven by a fixed linear dout, (out * w).sum(): the loss
  normalises by each rank's own positive count), and the replicas are bit-identical;
- a layer set frozen with freeze_batchnorm keeps its running statistics while the rest sync;
- negative control: the same ranks without the conversion differ from the full batch by far more than the tolerance.
The ranks get different query-length buckets (T 20 vs 50).  A further case runs unequal batches (1 + 3 images) without the DDP wrapper:
the all-reduced count N, not the world size, scales the statistics.  The configs[1] per-rank shape (R50-FPN at 300^2, 2 x 16 images on the
shipped tile table against 32 in one process) reaches every form of the lowering, and the test asserts that each occurred.  Every process group has a timeout and the children are joined with a
time limit, so a mismatched collective fails the test instead of hanging it."""
import datetime
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CASES = {
    # arch, image size, images per rank, freeze_batchnorm prefixes, DDP wrapper, small shape (ZSG_DETERMINISTIC=1, tolerances below)
    "r18_96_ddp_frozen": ("resnet18", 96, (2, 2), ("backbone.encoder.layer1.",), True, True),
    "r50_128_ddp": ("resnet50", 128, (2, 2), (), True, True),
    "r18_96_unequal": ("resnet18", 96, (1, 3), (), False, True),
    # configs[1] per-rank shape: R50-FPN at 300^2, 2 x B = 16 on the shipped tile table, against one process at B = 32 with the
    # library's heuristic tiles (ZSG_AUTOTUNE=0).  The shape that reaches every lowered form (see FORMS) — the deferred apply needs
    # activations of >= BN_PRE_MIN_MB — checked with the tolerances of test_gpu_fullshape.py / test_gpu_frozen_bn.py
    "configs1_r50_300_2x16": ("resnet50", 300, (16, 16), (), True, False),
}
# every form of the synchronized lowering that must occur at the configs[1] shape (plan.sync_bn_paths: forward form / backward form):
# statistics from a convolution's partial rows, the apply deferred into the next 1x1 convolution's loader, the stem pair, backward sums
# from a *_bnb data gradient, the plain backward pass, the residual gradient aliasing dout
FORMS = ("partials", "+bnpre", "/stem", "/bnb", "/plain", "+alias")


def _full_batch(B, S, seed):
    from oracle import zsg_oracle as O
    bt = O.synthetic_batch(B, S, S, T=50, seed=seed, tmax=50)
    q = bt["qlens"]
    q[: B // 2] = q[: B // 2].clamp(max=20)              # the first rank's queries fit the T = 20 bucket ...
    q[-1] = 50.0                                         # ... the last rank's need the T = 50 one
    return bt


def _net(arch, freeze):
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, mdl
    cfg = config.get_cfg(resnet_arch=arch)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict(arch, 17))
    net.to("cuda").train()
    if freeze:
        assert net.freeze_batchnorm(freeze)
    return net


def _inputs(full, a, b):
    T = 20 if float(full["qlens"][a:b].max()) <= 20 else 50
    inp = {k: v[a:b].cuda() for k, v in full.items()}
    inp["qvec"] = full["qvec"][a:b, :T].cuda()
    inp["h0"], inp["c0"] = torch.zeros(2, b - a, 128), torch.zeros(2, b - a, 128)
    return inp


def _dout(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _worker(rank, world, port, out_dir, name, tag="full"):
    arch, S, sizes, freeze, wrap, small = CASES[name]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if small:
        os.environ["ZSG_DETERMINISTIC"] = "1"
    elif world == 1:
        os.environ["ZSG_AUTOTUNE"] = "0"
        if tag == "full2":                               # the noise-floor twin: Winograd wherever it applies (another fp32 summation order)
            os.environ["ZSG_WINO"] = "force"
    import torch.distributed as dist
    from zsgnet_pytorch_amd import dist as zdist
    torch.cuda.set_device(0)
    net = _net(arch, freeze)
    full = _full_batch(sum(sizes), S, 5)
    if world == 1:                                       # the yardstick: one process, the concatenated batch
        inp = _inputs(full, 0, sum(sizes))
        out = net(inp)["att_bbx_out"]
        (out * _dout(out.shape, 9).cuda()).sum().backward()
        torch.cuda.synchronize()
        torch.save(dict(out=out.detach().cpu(), rmv=net._rmv.cpu().clone(), grad=net.store.grad.cpu().clone()), os.path.join(out_dir, tag + ".pt"))
        return
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    rmv0 = net._rmv.clone()
    model = zdist.DistributedDataParallel(net, device_ids=[0], broadcast_buffers=True, bucket_mb=1.0) if wrap else net
    assert zdist.convert_sync_batchnorm(model) is model
    a = sum(sizes[:rank])
    b = a + sizes[rank]
    inp = _inputs(full, a, b)
    out = model(inp)["att_bbx_out"]
    w = _dout((sum(sizes),) + tuple(out.shape[1:]), 9)[a:b].cuda()
    (out * w).sum().backward()
    torch.cuda.synchronize()
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    res = dict(out=out.detach().cpu(), rmv=net._rmv.cpu().clone(), rmv0=rmv0.cpu(), grad=net.store.grad.cpu().clone(),
               paths=dict(plan.sync_bn_paths), synced=sorted(plan.sync_bn), frozen=sorted(plan.frozen_bn),
               hosts=(sum(c[0].__name__ == "host" for c in plan.fwd.calls), sum(c[0].__name__ == "host" for c in plan.bwd.calls)))
    net.sync_batchnorm(enable=False)                     # negative control: per-rank statistics
    with torch.no_grad():
        res["out_unsynced"] = model(inp)["att_bbx_out"].detach().cpu()
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    if wrap:
        model.close()
    dist.destroy_process_group()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


@pytest.mark.parametrize("name", list(CASES))
def test_sync_batchnorm_matches_the_full_batch(tmp_path, name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    arch, S, sizes, freeze, wrap, small = CASES[name]
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), name)) for r in range(2)]
    procs.append(ctx.Process(target=_worker, args=(0, 1, port, str(tmp_path), name)))
    if not small:
        procs.append(ctx.Process(target=_worker, args=(0, 1, port, str(tmp_path), name, "full2")))
    for p in procs:
        p.start()
    for p in procs:
        p.join(420)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), f"a process failed or hung: {[p.exitcode for p in procs]}"
    r0, r1, ref = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt"), torch.load(tmp_path / "full.pt")
    n0 = sizes[0]
    # outputs: each rank's rows of the full batch
    e_out = max(_rel(r0["out"], ref["out"][:n0]), _rel(r1["out"], ref["out"][n0:]))
    assert e_out < 2e-3, e_out
    # negative control: per-rank statistics are far off
    e_neg = min(_rel(r0["out_unsynced"], ref["out"][:n0]), _rel(r1["out_unsynced"], ref["out"][n0:]))
    assert e_neg > 20 * 2e-3, (e_neg, e_out)
    # running statistics (mean | var of every layer): both ranks equal, and equal to the full batch's
    assert torch.equal(r0["rmv"], r1["rmv"])
    # (a running mean on the scale of its channel's batch standard deviation: a near-zero mean is a difference of large sums, and the
    # yardstick's convolutions sum in another order)
    nb = r0["rmv"].numel() // 2
    rmv, rv, rm0, rv0 = ref["rmv"].double(), ref["rmv"][nb:].double(), r0["rmv0"][:nb].double(), r0["rmv0"][nb:].double()
    bstd = ((rv - 0.9 * rv0) / 0.1).clamp(min=0).sqrt()
    scale = torch.cat([rmv[:nb].abs() + 0.1 * bstd + 1e-6, rmv[nb:].abs()])
    err = (r0["rmv"].double() - rmv).abs() / scale
    i = int(err.argmax())
    assert float(err[i]) < (1e-4 if small else 1e-3), (float(err[i]), i, float(r0["rmv"][i]), float(ref["rmv"][i]), float(r0["rmv0"][i]), e_out)
    # the synced layers are the train-mode ones; the frozen ones kept their running statistics
    assert r0["synced"] == r1["synced"] and len(r0["synced"]) > 0 and not set(r0["synced"]) & set(r0["frozen"])
    assert r0["hosts"] == (len(r0["synced"]), len(r0["synced"]))           # one collective per synced layer and direction
    assert set(r0["paths"]) == set(r0["synced"]) and all("/" in v for v in r0["paths"].values()), r0["paths"]
    print(name, "forms:", sorted(set(r0["paths"].values())))
    if not small:
        missing = [f for f in FORMS if not any(f in v for v in r0["paths"].values())]
        assert not missing, (missing, sorted(set(r0["paths"].values())))
        assert r0["paths"]["backbone.encoder.bn1"].endswith("/stem") and r0["hosts"] == (53, 53)
    from zsgnet_pytorch_amd import config, mdl
    net = mdl.get_default_net(9, config.get_cfg(resnet_arch=arch))
    if freeze:
        assert len(r0["frozen"]) > 0
        for nm in r0["frozen"]:
            L = net.bns[nm]
            nb = r0["rmv"].numel() // 2
            for off in (0, nb):
                sl = slice(off + L.index, off + L.index + L.c)
                assert torch.equal(r0["rmv"][sl], r0["rmv0"][sl]), nm
    # gradients: replicas bit-identical (wrapped); world x the reduced gradient (or the sum of the ranks' own) = the full batch's
    if wrap:
        assert torch.equal(r0["grad"], r1["grad"])
        g = 2 * r0["grad"]
    else:
        g = r0["grad"] + r1["grad"]
    # (the ranks and the yardstick tune their tiles apart and run other batch sizes: fp32 summation order differs, and through ResNet-50's
    # backward with 2 + 2 images that reaches ~2.4 % of the norm in the stem and layer1 — a wrong reduction is off by O(1).  2e-2 of the
    # largest element overall, 4e-2 of each parameter's gradient norm.  At configs[1] the yardstick's own fp32 noise is measured instead:
    # a twin of it with Winograd 3x3 convolutions (full2), and each parameter is held to test_gpu_net.grad_tol — as good as that twin (6x) or
    # within 1.5 % of the norm)
    ptol = 4e-2 if small else 1.5e-2
    ref2 = None if small else torch.load(tmp_path / "full2.pt")
    assert _rel(g, ref["grad"]) < 2e-2, _rel(g, ref["grad"])
    bad = []
    for n in net._param_names:
        e = net.store.entries[n]
        a, b = g[e.offset:e.offset + e.size].double(), ref["grad"][e.offset:e.offset + e.size].double()
        ec = 0.0
        if ref2 is not None:
            from test_gpu_net import grad_tol
            ec = float((ref2["grad"][e.offset:e.offset + e.size].double() - b).norm())
            tol = grad_tol(ec, b)
        else:
            tol = ptol * float(b.norm()) + 1e-9
        if float((a - b).norm()) > tol:
            bad.append((n, float((a - b).norm()) / (float(b.norm()) + 1e-30), ec / (float(b.norm()) + 1e-30)))
    assert not bad, bad[:8]

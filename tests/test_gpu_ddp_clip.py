"""Gradient clipping under data parallelism: two ranks sharing ONE GPU over gloo (as test_gpu_ddp_finetune.py).  With clipping engaged,
both ranks compute the same norm bits from the same all-reduced gradients, so their parameters stay bit-identical over three steps, and
the norm is the single-process norm of the averaged gradient."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

MAX_NORM = 0.02


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      ZSG_DETERMINISTIC="1")
    import torch.distributed as dist
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import config, dist as zdist, loss, mdl, optim
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 41))
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    ddp = zdist.DistributedDataParallel(net, device_ids=[0], broadcast_buffers=True, bucket_mb=1.0)
    opt = optim.FusedAdam(net, lr=1e-3)
    norms, grads = [], []
    for it in range(3):
        bt = {k: v.cuda() for k, v in O.synthetic_batch(2, 96, 96, seed=80 + 10 * it + rank).items()}
        bt["h0"], bt["c0"] = torch.zeros(2, 2, 128), torch.zeros(2, 2, 128)
        opt.zero_grad()
        lf(ddp(bt), bt)["loss"].backward()
        g = net.store.grad.clone()
        tn = optim.clip_grad_norm_(ddp.parameters(), MAX_NORM)
        opt.step()
        torch.cuda.synchronize()
        norms.append(tn.cpu())
        grads.append(g.cpu())
    torch.save(dict(norms=torch.stack(norms), grads=grads, w=net.store.flat.clone().cpu(), clipped=net.store.grad.clone().cpu()),
               os.path.join(out_dir, f"r{rank}.pt"))
    ddp.close()
    dist.destroy_process_group()


def test_two_rank_clip_keeps_replicas_identical(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, "a rank failed or hung"
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert torch.equal(a["norms"].view(torch.int32), b["norms"].view(torch.int32)), (a["norms"], b["norms"])
    assert torch.equal(a["w"].view(torch.int32), b["w"].view(torch.int32)), "the replicas' parameters drifted apart"
    for it in range(3):
        assert torch.equal(a["grads"][it], b["grads"][it])          # (the all-reduced gradient each rank clipped)
        ref = float(a["grads"][it].double().norm())                 # every parameter trains; padding holds zeros
        assert abs(float(a["norms"][it]) - ref) <= 1e-6 * ref, (float(a["norms"][it]), ref)
        assert ref > MAX_NORM                                       # clipping engaged
    cn = float(a["clipped"].double().norm())                        # the last step consumed max_norm * tn / (tn + 1e-6)
    assert MAX_NORM * (1 - 1e-3) <= cn <= MAX_NORM * (1 + 1e-6), cn

"""Synchronized BatchNorm, host side (no GPU): the `sync_bn` configuration key, dist.convert_sync_batchnorm without a process group and
on SSD-VGG (no BatchNorm layer: nothing to sync), and a gloo world-2 run in which both ranks create the BatchNorm collectives' own group
(dist.new_group, a collective call) without hanging."""
import datetime
import os
import socket

import torch.multiprocessing as mp


def _net(arch="resnet18", mdl_to_use="retina"):
    from zsgnet_pytorch_amd import config, mdl
    return mdl.get_default_net(9, config.get_cfg(resnet_arch=arch, mdl_to_use=mdl_to_use))


def test_sync_bn_config_key():
    from zsgnet_pytorch_amd import config
    assert config.get_cfg()["sync_bn"] is False
    assert config.get_cfg(sync_bn=True)["sync_bn"] is True


def test_convert_without_a_process_group_keeps_per_rank_statistics():
    from zsgnet_pytorch_amd import dist as zdist
    net = _net()
    assert zdist.convert_sync_batchnorm(net) is net
    assert net._sync_bn_group is None and net._sync_bn_key() == ()
    ssd = _net(mdl_to_use="ssd_vgg")
    assert zdist.convert_sync_batchnorm(ssd) is ssd and ssd._sync_bn_key() == () and not ssd.bns


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    from zsgnet_pytorch_amd import dist as zdist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    net = _net()
    net.freeze_batchnorm("backbone.encoder.layer4.")
    net.train()
    zdist.convert_sync_batchnorm(net)
    g = net._sync_bn_group
    assert g is not None and g is not dist.group.WORLD and dist.get_process_group_ranks(g) == [0, 1]
    key = net._sync_bn_key()
    assert len(key) == len(net.bns) - len(net._frozen_bn_key()) and not set(key) & set(net._frozen_bn_key())
    zdist.convert_sync_batchnorm(net)                    # the same group again: no second new_group
    assert net._sync_bn_group is g
    t = torch.full((3,), float(rank + 1), dtype=torch.float64)
    dist.all_reduce(t, group=g)
    assert t.tolist() == [3.0] * 3
    ssd = _net(mdl_to_use="ssd_vgg")                     # no BatchNorm: the conversion changes nothing
    zdist.convert_sync_batchnorm(ssd)
    assert ssd._sync_bn_key() == ()
    net.sync_batchnorm(enable=False)
    assert net._sync_bn_group is None and net._sync_bn_key() == ()
    with open(os.path.join(out, f"ok{rank}"), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_gloo_world2_creates_the_batchnorm_group(tmp_path):
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()

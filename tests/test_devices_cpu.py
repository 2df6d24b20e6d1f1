"""CPU: argument checks of StructureSolver(devices=, n_gpus=) that need no device."""
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devices_argument_errors():
    import blueberry_amd as bb
    S = bb.StructureSolver
    for kw, match in [(dict(devices=[]), "at least one"),
                      (dict(devices=[0, 0], device=0), "device"),
                      (dict(devices=[0, 1], n_gpus=2), "not both"),
                      (dict(n_gpus=2, device=1), "device"),
                      (dict(devices=[0, 0], distributed=True), "distributed"),
                      (dict(n_gpus=0), "positive"),
                      (dict(n_gpus=True), "positive"),
                      (dict(devices=[0, -1]), "non-negative"),
                      (dict(devices=[0, 1.5]), "non-negative"),
                      (dict(devices=[0] * 17), "16")]:
        with pytest.raises(ValueError, match=match):
            S(**kw)


def test_devices_forms():
    import blueberry_amd as bb
    assert bb.StructureSolver(n_gpus=3)._group == [0, 1, 2]
    assert bb.StructureSolver(devices=numpy.array([2, 2]))._group == [2, 2]
    one = bb.StructureSolver(devices=[1])
    assert one._group == [1] and one.device == 1            # one entry: as device=1
    assert bb.StructureSolver(n_gpus=1).device == 0
    assert bb.StructureSolver()._group is None


def test_devices_fit_many_is_refused_before_any_device_work():
    import blueberry_amd as bb
    with pytest.raises(ValueError, match="fit_many"):
        bb.StructureSolver(n_gpus=2).fit_many([numpy.ones((10, 10))])


def test_devices_inside_a_torch_distributed_job_is_refused():
    code = (
        "import sys, numpy\n"
        "sys.path.insert(0, %r)\n"
        "import torch.distributed as dist\n"
        "dist.init_process_group('gloo', init_method='tcp://127.0.0.1:0', rank=0, world_size=1)\n"
        "import blueberry_amd as bb\n"
        "for devices in ([0, 0], [0]):\n"
        "    try:\n"
        "        bb.StructureSolver(n_iter=1, devices=devices).fit(numpy.ones((20, 20)))\n"
        "    except ValueError as e:\n"
        "        assert 'torch.distributed' in str(e), e\n"
        "        print('refused', len(devices))\n"
        "dist.destroy_process_group()\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "refused 2" in r.stdout and "refused 1" in r.stdout, \
        r.stdout + r.stderr

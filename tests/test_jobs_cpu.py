"""CPU: the launcher of rank jobs (tests/_jobs.py) -- values in rank order, and on every way a
job can go wrong an error that names the rank, with no process left behind.  The workers are
trivial; no GPU is touched."""
import os
import time

import pytest

from tests import _jobs


def _none_alive():
    return len(_jobs.LAST) > 0 and not any(p.is_alive() for p in _jobs.LAST)


def _sum_worker(rank, world, base):
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    return base + rank, float(t[0])


@pytest.mark.parametrize("world", [1, 2, 3])
def test_values_come_back_in_rank_order(world):
    values = _jobs.run_ranks(_sum_worker, world, 10)
    assert values == [(10 + r, world * (world + 1) / 2.0) for r in range(world)]
    assert len(_jobs.LAST) == world and _none_alive()


def _raising_worker(rank, world):
    if rank == 1:
        raise ValueError("the scripted failure of this worker")
    return rank


def test_a_worker_that_raises_is_reported_with_its_rank_and_traceback():
    with pytest.raises(RuntimeError) as err:
        _jobs.run_ranks(_raising_worker, 2)
    assert "rank 1" in str(err.value) and "the scripted failure of this worker" in str(err.value)
    assert "ValueError" in str(err.value)
    assert _none_alive()


def _dying_worker(rank, world):
    if rank == 1:
        os._exit(3)
    import torch.distributed as dist
    dist.barrier()                       # rank 0 waits for a peer that is gone
    return rank


def test_a_process_that_dies_before_it_answers_ends_the_job_at_once():
    t0 = time.monotonic()
    with pytest.raises(RuntimeError) as err:
        _jobs.run_ranks(_dying_worker, 2, timeout=60)
    assert time.monotonic() - t0 < 30.0
    assert "rank 1" in str(err.value) and "code 3" in str(err.value)
    assert _none_alive()


def _sleeping_worker(rank, world):
    if rank == 0:
        time.sleep(600)
    return rank


def test_a_rank_that_gives_no_answer_is_named_and_killed():
    with pytest.raises(TimeoutError) as err:
        _jobs.run_ranks(_sleeping_worker, 2, timeout=3)
    assert "rank(s) 0" in str(err.value)
    assert _none_alive()


def _env_worker(rank, world):
    return os.environ.get("BB_JOBS_TEST_A"), os.environ.get("BB_JOBS_TEST_B")


def test_env_is_set_and_unset_in_every_rank(monkeypatch):
    monkeypatch.setenv("BB_JOBS_TEST_B", "set by the parent")
    monkeypatch.delenv("BB_JOBS_TEST_A", raising=False)
    values = _jobs.run_ranks(_env_worker, 2, env={"BB_JOBS_TEST_A": "1", "BB_JOBS_TEST_B": None})
    assert values == [("1", None), ("1", None)]
    assert _jobs.run_ranks(_env_worker, 1) == [(None, "set by the parent")]     # it was inherited


def _pending_worker(rank, world):
    import torch
    import torch.distributed as dist
    if rank == 0:
        dist.all_reduce(torch.zeros(1), async_op=True)      # nobody will ever complete it
    return rank * 7


def test_finish_exit_returns_the_values_and_every_process_exits_with_0():
    assert _jobs.run_ranks(_pending_worker, 2, finish="exit") == [0, 7]
    assert _none_alive()
    assert [p.exitcode for p in _jobs.LAST] == [0, 0]

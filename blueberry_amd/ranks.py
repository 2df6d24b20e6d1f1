"""Whether this process is a rank of a torch.distributed job, and what follows from it: the
job's (rank, world), the GPU to use when none is named, and the small collectives the host side
needs (an AND of outcomes, a sum of a host array, a gather of objects).  One probe answers the
first question and it never imports torch: a process that runs a job has imported it already, and
`import blueberry_amd` and the `devices=` path stay free of torch."""
import os
import sys

import numpy


def running_job():
    """The probe: `torch.distributed` when a job is initialised in this process, else None.
    torch is only looked at where the process has imported it already -- a process that runs a
    job has -- so nothing here ever pays for, or depends on, an import of torch."""
    dist = sys.modules.get("torch.distributed")
    if dist is not None and dist.is_available() and dist.is_initialized():
        return dist
    return None


def several_ranks():
    """Whether a job of more than one rank is running in this process."""
    dist = running_job()
    return dist is not None and dist.get_world_size() > 1


def pick_device(device, in_job):
    """The GPU to use: an explicit index wins; else this rank's own (LOCAL_RANK) where the
    caller is `in_job` -- an RCCL job must not put every rank's work on device 0 --, else 0."""
    if device is not None:
        return int(device)
    return int(os.environ.get("LOCAL_RANK", "0")) if in_job else 0


def dist_state(distributed):
    """(rank, world) of the running torch.distributed job, or (0, 1).  distributed None: a job
    is taken up where the probe finds one (importing torch just to find out costs the first
    fit() 0.7 s); False: never; anything else: there has to be one."""
    if distributed is False:
        return 0, 1
    if distributed is not None:
        import torch.distributed                  # noqa: F401 -- asked for: the probe then sees it
    dist = running_job()
    if dist is not None:
        return dist.get_rank(), dist.get_world_size()
    if distributed:
        raise RuntimeError("distributed=True but torch.distributed is not initialised")
    return 0, 1


def all_ranks(ok):
    """Collective AND over the ranks of one local outcome: every rank learns whether
    ALL of them succeeded, so that all of them take the same next step."""
    import torch.distributed as dist
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, bool(ok))
    return all(flags)


def sum_over_ranks(counts, eng, world):
    """Element-wise sum of an int64 host array over the ranks (world 1: the array); a float
    array is summed in float64 (the weighted degrees of SPEC 2.4.1)."""
    if world <= 1:
        return counts
    import torch
    import torch.distributed as dist
    kind = numpy.float64 if numpy.asarray(counts).dtype.kind == "f" else numpy.int64
    t = torch.from_numpy(numpy.ascontiguousarray(counts, dtype=kind))
    if dist.get_backend() == "nccl":
        t = t.to(torch.device("cuda", eng.device))
        dist.all_reduce(t)
        return t.cpu().numpy()
    dist.all_reduce(t)
    return t.numpy()


def gather_objects(obj, world):
    """Every rank's `obj`, in rank order, on every rank (`all_gather_object`).  Collective."""
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, obj)
    return parts

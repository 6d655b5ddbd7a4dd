"""The pipe forms of the five control-plane stages (ICMP replies, received ICMP errors, ARP replies, the IGMP
responder, neighbour learning) through the C ABI, for what they share: which pipes they take, what the stats call
says before any run, and what an empty batch leaves. What each stage computes is its own tests' business."""
import ctypes as C
import errno

import numpy as np
import pytest

import arp_util as A
import icmp_util as I
import neigh_util as N
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

MAX_PIPES = 4
LISTS = {abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}


class _Form:
    """One stage's pipe form on a context: run(pipe) enqueues an empty batch, stats(pipe) -> (rc, struct)."""

    def __init__(self, ctx, stage):
        L, self.ctx, self.stage = abi.lib(), ctx, stage
        can = lambda nbytes: ctx.upload(np.full(nbytes, 0xA5, np.uint8))
        self.bufs = [ctx.upload(np.zeros(1, np.uint32)), can(256), can(64), can(64)]   # meta, then outputs
        meta, out, aux, aux2 = (C.c_void_p(b.ptr) for b in self.bufs)
        self.bt = abi.RxBatch(None, 0, None, None, None, 0)
        bt = C.byref(self.bt)
        if stage == "icmp":
            self.cfg, self.o = I.tx_config(), abi.IcmpOut(out.value, 192, aux.value, aux2.value, 4)
            self.run = lambda p: L.udpdk_gpu_pipe_icmp_reply(ctx.handle, p, C.byref(self.cfg), bt, meta, abi.ICMP_ALL, 0,
                                                             0xFFFFFFFF, C.byref(self.o))
            self.st, fn = abi.IcmpStats(), L.udpdk_gpu_pipe_icmp_stats
        elif stage == "icmp_err":
            ctx.upload_snapshot(abi.snapshot_from_lists(LISTS, 1))
            self.run = lambda p: L.udpdk_gpu_pipe_icmp_errors(ctx.handle, p, abi.raw_ip(A.OUR_IP), bt, meta, aux, 1, out)
            self.st, fn = abi.IcmpErrStats(), L.udpdk_gpu_pipe_icmp_err_stats
        elif stage == "arp":
            self.cfg, self.o = A.tx_config(), abi.ArpOut(out.value, aux.value, 4)
            self.run = lambda p: L.udpdk_gpu_pipe_arp_reply(ctx.handle, p, C.byref(self.cfg), bt, meta, C.byref(self.o))
            self.st, fn = abi.ArpStats(), L.udpdk_gpu_pipe_arp_stats
        elif stage == "igmp":
            self.cfg, self.o = A.tx_config(), abi.IgmpOut(out.value, aux.value, 4)
            self.run = lambda p: L.udpdk_gpu_pipe_igmp_reply(ctx.handle, p, C.byref(self.cfg), bt, meta, None, 0,
                                                             C.byref(self.o))
            self.st, fn = abi.IgmpStats(), L.udpdk_gpu_pipe_igmp_stats
        else:
            assert stage == "neigh_learn" and abi.neigh_create(ctx, 8) == 0
            self.cfg = N.cfg()
            self.run = lambda p: L.udpdk_gpu_pipe_neigh_learn(ctx.handle, p, C.byref(self.cfg), bt, meta, 7)
            self.st, fn = abi.NeighLearnStats(), L.udpdk_gpu_pipe_neigh_learn_stats
        self.stats = lambda p: fn(ctx.handle, p, C.byref(self.st))

    def fields(self):
        return {f[0]: getattr(self.st, f[0]) for f in self.st._fields_}


@pytest.fixture(params=["icmp", "icmp_err", "arp", "igmp", "neigh_learn"])
def form(request):
    with abi.GpuContext(0, max_frames=1024, max_lanes=8) as ctx:
        ctx.pipeline(2)
        f = _Form(ctx, request.param)
        yield f
        ctx.sync()
        for b in f.bufs:
            b.free()


def test_stats_before_any_run(form):
    for pipe in range(1, MAX_PIPES):
        assert form.stats(pipe) == -errno.ENOENT, pipe


def test_pipes_out_of_range(form):
    for pipe in (0, MAX_PIPES, -1):
        assert form.run(pipe) == -errno.EINVAL, pipe
        assert form.stats(pipe) == -errno.EINVAL, pipe
    for pipe in range(1, MAX_PIPES):                               # and nothing ran anywhere
        assert form.stats(pipe) == -errno.ENOENT, pipe


def test_empty_batch(form):
    L = abi.lib()
    assert form.run(1) == 0
    assert L.udpdk_gpu_pipe_wait(form.ctx.handle, 1) == 0
    for f in form.st._fields_:                                     # whatever the call leaves must come from the stage
        setattr(form.st, f[0], 0x5A)
    assert form.stats(1) == 0
    assert form.fields() == {f[0]: 0 for f in form.st._fields_}
    assert form.stats(2) == -errno.ENOENT                          # the other pipes' slots are their own

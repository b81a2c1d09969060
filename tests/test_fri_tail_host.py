"""The tail form of the FRI commit phase, host side, without a device: the two entry points are declared, exported and bound,
their refusals come before any device work, and Chain keeps its fri_tail_log."""
import ctypes
import os
import re

import numpy as np

NEW = ("rsv_fri_commit_tail_dev", "rsv_witness_fri_tail_dev")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsv.h")


def test_entry_points_are_declared_exported_and_bound(rsv):
    with open(HEADER) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in rsv.EXPORTS and hasattr(rsv.lib, name), name
    assert re.search(r"^#define RSV_MAX_FRI_TAIL_LOG 10$", header, re.M)
    assert rsv.lib.rsv_abi_version() == 6


def test_refusals_need_no_device(rsv):
    """A NULL context gives RSV_E_NULL; every refusal of the cap forms comes back in its order, then tail_log: a context that
    is zero bytes and device pointers that are plain numbers are never dereferenced."""
    lib = rsv.lib
    ctx = ctypes.cast(ctypes.create_string_buffer(8192), ctypes.c_void_p)
    prog = ctypes.cast(ctypes.create_string_buffer(8192), ctypes.c_void_p)
    buf, odd = ctypes.c_void_p(8192), ctypes.c_void_p(8194)

    def commit(ctx=ctx, quot=buf, sizes=(5,), b=1, last=1, n=1, chan=buf, roots=buf, alphas=buf, layers=buf, poly=buf, low=buf, h=3, caps=buf, t=4):
        keep = np.array(sizes, np.uint32)
        return lib.rsv_fri_commit_tail_dev(ctx, quot, keep.ctypes.data_as(rsv._u32p), len(keep), b, last, n, None, chan, roots, alphas, layers, poly,
                                           low, h, caps, t)

    for t in (0, 4, 11):
        for k in ("ctx", "quot", "chan", "roots", "alphas", "layers", "poly", "low"):
            assert commit(**{k: None}, t=t) == -1, (k, t)
        for kw in ({"sizes": (5, 5)}, {"sizes": (5, 6)}, {"sizes": (31,)}, {"last": 4}, {"b": 0}, {"n": (1 << 20) + 1}, {"h": 0}, {"h": 9}, {"caps": odd},
                   {"quot": odd}, {"layers": odd}):
            assert commit(**kw, t=t) == -2, (kw, t)
    assert commit(t=11) == -2 and commit(t=11, caps=None, h=0) == -2
    assert commit(quot=None, t=11) == -1  # a NULL comes before tail_log
    assert commit(n=0) == 0 and commit(n=0, t=0) == 0  # an empty batch is no work
    assert commit(caps=None, h=77, sizes=(5, 5)) == -2 and commit(caps=None, h=77, quot=None) == -1  # d_caps NULL: sub_log is not read

    def chain(ctx=ctx, prog=prog, plonk=buf, comp=buf, chan=buf, quot=buf, roots=buf, layers=buf, h=3, caps=buf, n=1, t=4):
        return lib.rsv_witness_fri_tail_dev(ctx, prog, plonk, buf, buf, buf, buf, buf, None, n, 1, 0, comp, buf, buf, buf, chan, buf, quot, roots, buf,
                                            layers, buf, buf, h, caps, t)

    for t in (0, 4, 11):
        for k in ("ctx", "prog", "plonk", "comp", "chan", "quot", "roots"):
            assert chain(**{k: None}, t=t) == -1, (k, t)
        for kw in ({"h": 0}, {"h": 9}, {"caps": odd}, {"quot": odd}, {"n": (1 << 20) + 1}):
            assert chain(**kw, t=t) == -2, (kw, t)
    assert chain() == -2 and chain(t=11) == -2  # a program that was not built
    if rsv.device_count() == 0:
        assert commit() == -3 and commit(t=10, sizes=(7, 6, 5), last=2) == -3 and commit(t=0) == -3


def test_chain_stores_fri_tail_log(rsv):
    class Program:
        def trace_sizes(self):
            return 5, 6

        def gates(self):
            return [], []

    ch = rsv.Chain(None, Program(), 1, 1, log_last=0, fri_sub_log=8, fri_tail_log=10)
    assert (ch.fri_tail_log, ch.fri_sub_log) == (10, 8)
    assert rsv.Chain(None, Program(), 1, 1).fri_tail_log == 0

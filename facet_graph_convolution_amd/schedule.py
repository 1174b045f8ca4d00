"""The schedule protocol: what a step's generator yields, who serves it, and how a schedule becomes hipGraph segments.

A schedule (FacetDenoiser._forward_gen, _loss_backward_gen, ...) enqueues launches and YIELDS a request wherever a
facet-sharded run must talk to its peers; an unsharded run yields nothing.  The four requests:
  Xchg(items, key)   ONE grouped exchange with every peer (shard.PackedExchange); items:
       Rows(level, tensor, parent)    halo rows of `tensor` (parent: the rows of the coarse parents)
       PEdges(level, tensor)          per-pair rows (dt, d-logits) of the pairs whose parent a peer owns
       Edges(level)                   d-logits of incoming cross-shard edges
     key None: blocking.  Otherwise the kernels enqueued up to the matching Wait(key) run while it travels
  Wait(key)          the exchange begun under `key` has to have landed
  Sum(tensor)        all-reduce
  Call(fn)           launches whose arguments change from step to step (a rank's own loss samples): run by an eager
                     call, also between the hipGraphs of a captured schedule
Every type keeps a constant kind string in field 0.  `serve` runs a request through a communicator (shard.DistComm);
shard.sim_run serves the same requests among simulated shards.  A SEGMENT is (hipGraph or None, request or None): the
launches of one stretch between two requests, and the request that ends the stretch (`capture_segments`, `replay`).
"""
import collections
import contextlib
import ctypes as C
import functools
import gc
import os
import warnings

import torch


def _kind(name, kind, fields, defaults=()):
    """(the namedtuple `name` with the constant `kind` in field 0, its constructor of the other fields)"""
    T = collections.namedtuple(name, "kind " + fields, defaults=defaults)
    return T, functools.partial(T, kind)


Xchg, xchg = _kind("Xchg", "xchg", "items key", (None,))
Wait, wait = _kind("Wait", "wait", "key")
Sum, sum_ = _kind("Sum", "sum", "tensor")
Call, call = _kind("Call", "call", "fn")
Rows, rows = _kind("Rows", "rows", "level tensor parent", (False,))
PEdges, pedges = _kind("PEdges", "pedges", "level tensor")
Edges, edges = _kind("Edges", "edges", "level")
_REQUESTS = {"xchg": Xchg, "wait": Wait, "sum": Sum, "call": Call}


def named(req):
    """`req` as its named type: a hand-written schedule (tests, probes) may yield bare tuples in the field order."""
    return req if hasattr(req, "kind") else _REQUESTS[req[0]](*req)


def serve(req, comm, packed_of, pending):
    """One request of a schedule through `comm` (exchange now / begin / await, or an all-reduce).  packed_of(req): the
    PackedExchange of an Xchg; pending: {key: handle} of the exchanges in flight."""
    kind = req.kind
    if kind == "wait":
        comm.finish(pending.pop(req.key))
    elif kind == "call":
        req.fn()
    elif kind == "sum":
        comm.all_reduce_sum(req.tensor)
    else:
        px = packed_of(req)
        if req.key is None:
            comm.exchange(px)
        else:
            pending[req.key] = comm.exchange_begin(px)


def drain(gen, comm, packed_of):
    """Run a schedule on this rank: nothing to serve when unsharded, collectives through `comm` otherwise."""
    pending = {}
    for req in gen:
        serve(req, comm, packed_of, pending)


_HIP = [None]


def _graph_node_count(g):
    """Nodes of a captured (not yet instantiated) torch.cuda.CUDAGraph(keep_graph=True), through hipGraphGetNodes.  Raises
    when the runtime cannot say: whether a stretch of the schedule is a graph at all must not be a guess."""
    if _HIP[0] is None:
        _HIP[0] = C.CDLL("libamdhip64.so")
    n = C.c_size_t(0)
    rc = _HIP[0].hipGraphGetNodes(C.c_void_p(g.raw_cuda_graph()), None, C.byref(n))
    if rc != 0:
        raise RuntimeError("hipGraphGetNodes failed (%d): cannot tell whether a schedule segment has launches" % rc)
    return int(n.value)


@contextlib.contextmanager
def _no_gc_while_capturing():
    """A stream capture must not be interrupted by Python's cyclic garbage collector.  A dead reference cycle that still owns
    device objects - the hipGraphs and pool tensors of an earlier network, say - is freed whenever the collector happens to
    run, and it runs on allocation counts: in the middle of a capture its destructors call hipGraphDestroy / hipFree, which
    a capturing stream refuses; torch raises from a destructor and the process ABORTS (the round-3 abort, caught in round 4
    with its stack: `Garbage-collecting` under `_capture_segments`).  torch.cuda.graph stopped
    collecting in its __enter__ (torch.compiler.config.force_cudagraph_gc, default off), so: collect once before the
    capture, keep the collector off until it has ended.  FGC_NO_CAPTURE_GC_GUARD=1 (developer switch): no guard."""
    if os.environ.get("FGC_NO_CAPTURE_GC_GUARD", "0") == "1":
        yield
        return
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def capture_segments(make_gen):
    """A facet-sharded schedule as a list of segments (hipGraph, request): the launches between two exchanges are captured
    into one graph each; the exchanges themselves (row gather + grouped point-to-point, all-reduces) stay eager
    calls between the replays - a collective is not a graph node here.  The schedule is static (same buffers, same
    tile lists, same message sizes every step), so the requests recorded with the graphs are replayed as they are.
    Returns (segments, the node count of each)."""
    # (one collection in front of the first capture, the collector off until the last one has ended: a full collection
    #  per segment - thirty a step and shard - made the capture of an 8-shard step take seconds)
    with _no_gc_while_capturing():
        gen = make_gen()
        segs, counts = [], []
        while True:
            g = torch.cuda.CUDAGraph(keep_graph=True)
            # (thread_local: the collective back end's watchdog thread may query its events while this thread captures)
            # Whether a stretch has launches is only known once it has been captured - library launches and torch
            # operations alike become nodes, and nothing else sees both - so a stretch of two requests back to back IS
            # captured; torch's "The CUDA Graph is empty" warning about it is expected here and silenced for exactly
            # these captures (the graph is dropped below: never instantiated, never replayed).
            with warnings.catch_warnings():
                warnings.filterwarnings("ignore", message="The CUDA Graph is empty")
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    try:
                        req = next(gen)
                    except StopIteration:
                        req = None
            # a stretch WITHOUT launches (two requests back to back, or nothing behind the last one) is no graph at all:
            # an empty hipGraph is never instantiated or replayed (the counts are kept for the tests)
            nodes = _graph_node_count(g)
            if nodes == 0:
                g = None
            else:
                g.instantiate()
            counts.append(nodes)
            segs.append((g, req))
            if req is None:
                return segs, counts


def replay(segs):
    """The schedule recorded in `segs`: replays each graph and yields each recorded request."""
    for g, req in segs:
        if g is not None:        # (a stretch without launches is no graph: capture_segments)
            g.replay()
        if req is not None:
            yield req

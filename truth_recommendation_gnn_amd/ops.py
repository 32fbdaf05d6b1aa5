"""Autograd operators over the HIP kernels.

``hetero_layer`` is one full SAGE layer over every destination node type at once — the fused
form of ``WeightedRGCN.forward`` (``train_gnn.py:166-200``):

    y_dst = act( sum_r w_r * (mean_{src->dst} x_src @ W_l,r^T + b_r + x_dst @ W_r,r^T) )

computed as: K1 ``gather_mean`` per relation, then ONE K3 multi-segment MFMA linear per
destination over ``[aggr_1 .. aggr_R, x_dst]`` with the K-concatenated, relation-weighted
weights (built by torch ops on the parameters, so autograd routes the gradients back to the
reference's own per-conv parameters).  Backward: K3 dgrad/wgrad (ReLU mask fused), then K2
``scatter_mean_bwd`` accumulating straight into the source-feature gradients, so the per-type
gradient sums the reference's autograd would do with separate add kernels happen in-kernel.
"""
from __future__ import annotations

import dataclasses
import math
import os
import weakref
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _native as N
from .graph import RelationCSR


def _check_f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: hgnn computes in fp32 (the reference dtype); got {t.dtype}")
    return t.contiguous()


# ----------------------------------------------------------------------------- row storage
# How the forward gathers and the link loss store the rows they read once per edge from a layer
# output.  "fp32" (the default): the tables themselves, the fp32 parity path.  "bf16" (opt-in):
# a bf16 copy of each such table (``rows_to_bf16``, round to nearest even), half the row bytes;
# every result is then what the fp32 path gives on R(T) = T.to(bfloat16).float(), gradients pass
# straight through R, and everything that is not a gathered row stays fp32.
# Read from HGNN_ROW_DTYPE at import, as HGNN_HOT_ROWS / HGNN_STATIC_AGG are; a LayerSpec, the
# model constructors and the loss take a ``row_dtype`` of their own, None meaning this value at
# call time.
ROW_DTYPES = ("fp32", "bf16")


def _row_dtype_value(v: str, what: str) -> str:
    if v not in ROW_DTYPES:
        raise ValueError(f"{what}={v!r}: the row storage is 'fp32' or 'bf16'")
    return v


ROW_DTYPE = _row_dtype_value(os.environ.get("HGNN_ROW_DTYPE", "fp32"), "HGNN_ROW_DTYPE")


def resolve_row_dtype(row_dtype: Optional[str]) -> str:
    """``row_dtype`` itself, or the module's ``ROW_DTYPE`` (as it is now) for None."""
    return _row_dtype_value(ROW_DTYPE if row_dtype is None else row_dtype, "row_dtype")


# How the backward's K2 scatters store the gradient rows they read once per edge, a second
# opt-in independent of ROW_DTYPE.  "fp32" (the default): the fp32 gradient tables themselves.
# "bf16": each K2 of a fused layer's backward reads a bf16 copy of its table — the K3 dgrad's
# dA of an aggregate segment (``rows_to_bf16``), or a pre-projected relation's ReLU-masked dz
# (``relu_grad_bf16``, the mask fused into the cast) — so every gradient the layer returns is what
# the fp32 backward gives when each K2 reads R(T) in place of T.  K2's accumulators and outputs,
# K3, the weight, bias and root gradients stay fp32.  Read from
# HGNN_GRAD_ROW_DTYPE at import; a LayerSpec and the model constructors take a ``grad_row_dtype``
# of their own, None meaning this value at call time.
GRAD_ROW_DTYPE = _row_dtype_value(os.environ.get("HGNN_GRAD_ROW_DTYPE", "fp32"),
                                  "HGNN_GRAD_ROW_DTYPE")


def resolve_grad_row_dtype(grad_row_dtype: Optional[str]) -> str:
    """``grad_row_dtype`` itself, or the module's ``GRAD_ROW_DTYPE`` (as it is now) for None."""
    return _row_dtype_value(GRAD_ROW_DTYPE if grad_row_dtype is None else grad_row_dtype,
                            "grad_row_dtype")


# ----------------------------------------------------------------------------- kernel timing
class KernelTimer:
    """Records HIP events around every kernel call this module makes (on the current stream,
    the one the kernels are launched on), with each launch's algorithmic HBM bytes.  Used by
    bench.py inside its timed region; ``None`` when off (zero overhead)."""

    def __init__(self):
        # (name, algorithmic bytes, start event, end event, compulsory bytes, flops)
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, nbytes, s, e, cbytes, flops in self.records:
            ms = s.elapsed_time(e)
            a = agg.setdefault(name, {"launches": 0, "ms": 0.0, "bytes": 0, "cbytes": 0,
                                      "flops": 0})
            a["launches"] += 1
            a["ms"] += ms
            a["bytes"] += nbytes
            a["cbytes"] += cbytes
            a["flops"] += flops
        return agg


_timer: Optional[KernelTimer] = None


def set_timer(t: Optional[KernelTimer]) -> None:
    global _timer
    _timer = t


class _timed:
    """``cbytes``: compulsory bytes (every table row counted once), when it differs from the
    algorithmic figure — the honest number for a gather whose source table is cache-resident.
    ``flops``: algorithmic flops of an MFMA kernel (K3), 0 elsewhere."""

    def __init__(self, name, nbytes, cbytes=None, flops=0):
        self.name, self.nbytes, self.flops = name, nbytes, flops
        self.cbytes = nbytes if cbytes is None else cbytes

    def __enter__(self):
        if _timer is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if _timer is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _timer.records.append((self.name, int(self.nbytes), self.s, e, int(self.cbytes),
                                   int(self.flops)))


def gather_bytes(n_edges: int, n_rows: int, d: int, weighted: bool,
                 row_bytes: Optional[int] = None) -> int:
    """Algorithmic HBM bytes of one K1/K2 launch: per edge a 4-B index and one
    source row of ``row_bytes`` (4*d for fp32 rows, the default; 2*d for bf16 rows) (+4 B weight
    for K2), rowptr, and the fp32 output rows."""
    rb = 4 * d if row_bytes is None else int(row_bytes)
    return (n_edges * (4 + rb + (4 if weighted else 0)) + 4 * (n_rows + 1) + 4 * n_rows * d)


def gather_compulsory_bytes(n_edges: int, n_rows: int, n_src: int, d: int, weighted: bool,
                            row_bytes: Optional[int] = None) -> int:
    """As gather_bytes with each source row read once: min(E, N_src) rows instead of E."""
    rb = 4 * d if row_bytes is None else int(row_bytes)
    return (4 * n_edges * (1 + (1 if weighted else 0)) + min(n_edges, n_src) * rb
            + 4 * (n_rows + 1) + 4 * n_rows * d)


def _row_bytes(x: torch.Tensor) -> int:
    return int(x.shape[1]) * x.element_size()


def rows_to_bf16(x: torch.Tensor) -> torch.Tensor:
    """The bf16 copy of an fp32 tensor (``hgnn_rows_to_bf16``): round to nearest even, bitwise
    ``x.to(torch.bfloat16)``.  One streaming pass; the row mode's shadow tables."""
    x = _check_f32(x, "rows_to_bf16")
    dev = N.require_device(x)
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
    name = f"rows_to_bf16[{x.shape[0]}]x{x.shape[1]}" if x.dim() == 2 else "rows_to_bf16"
    with _timed(name, 6 * x.numel()):
        N.check(N.lib().hgnn_rows_to_bf16(N.ptr(x), x.numel(), N.ptr(out), N.stream_ptr(dev)),
                "hgnn_rows_to_bf16")
    return out


def relu_grad_bf16(dout: torch.Tensor, out_act: Optional[torch.Tensor] = None,
                   mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bf16(dout * (out > 0))`` in one streaming pass (``hgnn_relu_grad_to_bf16``): ReLU's
    backward fused into the cast, bitwise ``rows_to_bf16`` of the ``dz_out`` the K3 backward
    writes.  The predicate is exactly one of ``out_act`` (the forward's output) and ``mask`` (its
    ReLU bits, :func:`relu_mask_for`; 16 B read per row instead of the 4h-byte output)."""
    dout = _check_f32(dout, "relu_grad_bf16")
    if dout.dim() != 2:
        raise ValueError(f"relu_grad_bf16: dout is {tuple(dout.shape)}, expected [n, h]")
    n, h = int(dout.shape[0]), int(dout.shape[1])
    if out_act is not None:
        out_act = _check_f32(out_act, "relu_grad_bf16")
        if tuple(out_act.shape) != (n, h):
            raise ValueError(f"relu_grad_bf16: out_act is {tuple(out_act.shape)}, "
                             f"expected {(n, h)}")
    if mask is not None and (mask.dtype != torch.int32 or tuple(mask.shape) != (n, 4)
                             or not mask.is_contiguous()):
        raise ValueError(f"relu_grad_bf16: ReLU bits are {mask.dtype} {tuple(mask.shape)}, "
                         f"expected contiguous int32 {(n, 4)}")
    dev = N.require_device(dout, out_act, mask)
    dz = torch.empty((n, h), dtype=torch.bfloat16, device=dev)
    nbytes = 6 * n * h + 16 * n if mask is not None else 10 * n * h
    with _timed(f"relu_grad_bf16[{n}]x{h}", nbytes):
        N.check(N.lib().hgnn_relu_grad_to_bf16(N.ptr(dout), N.ptr(out_act), N.ptr(mask), n, h,
                                               N.ptr(dz), N.stream_ptr(dev)),
                "hgnn_relu_grad_to_bf16")
    return dz


def _check_table(t: torch.Tensor, what: str) -> torch.Tensor:
    """A gather's source table: fp32, or the bf16 rows of the row mode."""
    if t.dtype == torch.bfloat16:
        return t.contiguous()
    return _check_f32(t, what)


# ----------------------------------------------------------------------------- raw kernel calls
# Source-blocked gathers.  Random rows from a table of several GB come back at ~6.3 TB/s; the
# same rows from a ~600 MB slice of it at ~7.2 TB/s (cfg4 K1 post<-user, scripts/ic_block_bench.py:
# 16.96 ms in one pass, 15.36 ms in 8 passes over 575-MB user blocks, each pass adding its block's
# sum into the output).  The passes re-read and re-write the output (B-1 extra round trips of
# N_dst x 4d bytes), which the gain pays for only while the blocks stay large: 8 passes is the
# best measured split of a 4.6 GB table, 16 is already even.  So a gather whose source table is
# at least GATHER_BLOCK_BYTES is split into ceil(table / GATHER_BLOCK_SLICE) passes.
GATHER_BLOCK_BYTES = int(float(os.environ.get("HGNN_GATHER_BLOCK_GB", "2")) * 2**30)
GATHER_BLOCK_SLICE = int(float(os.environ.get("HGNN_GATHER_BLOCK_MB", "600")) * 2**20)


def gather_blocks(x: torch.Tensor, n_edges: Optional[int] = None) -> int:
    """Number of source-block passes for a gather reading table ``x`` (1: one plain pass).  A
    gather of fewer edges than the table has rows (a sampled block reading the global tables)
    reads a thin random subset at latency-bound rates, where the passes' locality buys nothing
    and their (block, row) CSR would cost a sort per block: one pass."""
    nbytes = x.numel() * x.element_size()
    if GATHER_BLOCK_BYTES <= 0 or nbytes < GATHER_BLOCK_BYTES:
        return 1
    if n_edges is not None and n_edges < x.shape[0]:
        return 1
    return int(-(-nbytes // GATHER_BLOCK_SLICE))


class _PlanArgs(tuple):
    """``_plan_args``' result; it also holds the slab: keep it until the launch is enqueued."""


def _plan_args(p, d: int, dev) -> _PlanArgs:
    """``(heavy_rows, heavy_first, n_heavy, n_chunks, chunk, slab)`` in ABI order for a gather of
    ``d`` columns; the slab (the heavy rows' partial sums) is allocated when there are any."""
    slab = torch.empty(p.n_chunks * d, dtype=torch.float32, device=dev) if p.n_heavy else None
    args = _PlanArgs((N.ptr(p.heavy_rows), N.ptr(p.heavy_first), p.n_heavy, p.n_chunks, p.chunk,
                      N.ptr(slab)))
    args.slab = slab
    return args


def _launch_gather(x, g, edge_w, col_w, row_w, flags, out, hot=None):
    """One K1 / K2 launch over grouping ``g`` through the entry point that the table's dtype,
    ``hot`` (the grouping's ``graph.HotCols``: two-policy row loads, same sums) and ``row_w`` (a
    per-row scale in place of the mean) select."""
    d = int(out.shape[1])
    dev = out.device
    lib, s = N.lib(), N.stream_ptr(dev)
    plan = _plan_args(g.plan, d, dev)
    head = (N.ptr(x), x.shape[0], d, N.ptr(g.rowptr), N.ptr(g.col), g.n_rows, N.ptr(edge_w),
            N.ptr(col_w))
    if x.dtype == torch.bfloat16:
        N.check(lib.hgnn_gather_reduce_bf16(
            *head, N.ptr(row_w), flags, *plan, N.ptr(out), 0,
            N.ptr(hot.col) if hot is not None else None, hot.share if hot is not None else 0.0,
            s), "hgnn_gather_reduce_bf16")
    elif row_w is not None:     # (the source-blocked passes: no caller has hot columns for them)
        N.check(lib.hgnn_gather_reduce_scaled(*head, N.ptr(row_w), flags, *plan, N.ptr(out), s),
                "hgnn_gather_reduce_scaled")
    elif hot is not None:
        N.check(lib.hgnn_gather_reduce_hot(*head, flags, *plan, N.ptr(out), 0, N.ptr(hot.col),
                                           hot.share, s), "hgnn_gather_reduce_hot")
    else:
        N.check(lib.hgnn_gather_reduce(*head, flags, *plan, N.ptr(out), s), "hgnn_gather_reduce")


def _gather_blocked(x, passes, row_w, edge_w, out, accumulate, name, nbytes, cbytes):
    """All passes of a source-blocked gather, timed as one gather (its algorithmic bytes are the
    unblocked gather's)."""
    with _timed(name, nbytes, cbytes):
        for b, g in enumerate(passes):
            flags = N.HGNN_ACCUMULATE if (accumulate or b > 0) else 0
            _launch_gather(x, g, edge_w, None, row_w, flags, out)


# ----------------------------------------------------------------------------- static aggregates
# The mean of a model INPUT table over a relation is the same every step (the reference builds
# x_dict once, train_gnn.py:87-88,118-119, and passes it unchanged to every epoch's forward and
# to evaluation, :254,391,424).  A caller that knows a table is such an input says so
# (``gather_mean(..., static=True)``; nn.HeteroSAGE / the layout models at their first layer) and
# the aggregate is computed once and kept on the RelationCSR — at cfg4 a 200M-edge gather per
# direction (~205 GB of random row reads per step) for 5.1 GB held.  Nothing here guesses: an
# unflagged call always runs its kernel.
#
# HGNN_STATIC_AGG: "1" (default) keep them; "0" never; "check" keep them and verify the table's
# checksum (hgnn_table_fingerprint, one streaming pass over the table) on every hit.
STATIC_AGG = os.environ.get("HGNN_STATIC_AGG", "1")
_STATIC_HOLDERS: "weakref.WeakSet" = weakref.WeakSet()   # RelationCSRs holding an entry


class StaleAggregateError(RuntimeError):
    """HGNN_STATIC_AGG=check: a table's memory changed under a kept aggregate."""


class _StaticEntry:
    """One kept aggregate: the table it was computed from (weakly), what identifies the table's
    contents (pointer, shape, strides, version counter, the blocking the gather ran with), the
    aggregate, and under ``check`` the table's fingerprint (a device int64)."""
    __slots__ = ("ref", "key", "value", "fp", "event", "stream", "fin", "__weakref__")

    def __init__(self, x, key, value, fp):
        self.ref, self.key, self.value, self.fp = weakref.ref(x), key, value, fp
        self.event = self.stream = self.fin = None
        if value.is_cuda:
            # a hit on another stream waits for the fill (same stream: in order already)
            self.stream = torch.cuda.current_stream(value.device)
            self.event = torch.cuda.Event()
            self.event.record(self.stream)


def _static_key(x: torch.Tensor, blocks: int):
    return (x.data_ptr(), tuple(x.shape), tuple(x.stride()), x._version, int(blocks))


def table_fingerprint(x: torch.Tensor) -> torch.Tensor:
    """``hgnn_table_fingerprint`` of a contiguous fp32 tensor: a device int64 holding the 64-bit
    checksum's bits (no host sync)."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("table_fingerprint: a contiguous float32 tensor")
    dev = N.require_device(x)
    out = torch.empty(1, dtype=torch.int64, device=dev)
    with _timed("table_fingerprint", 4 * x.numel()):
        N.check(N.lib().hgnn_table_fingerprint(N.ptr(x), x.numel(), N.ptr(out),
                                               N.stream_ptr(dev)), "hgnn_table_fingerprint")
    return out


def _static_enabled(x: torch.Tensor) -> bool:
    if STATIC_AGG == "0":
        return False
    # a recorded graph must hold its own kernels: nothing is kept from, or served into, a capture
    return not (x.is_cuda and torch.cuda.is_current_stream_capturing())


def _static_drop(csr_ref, entry_ref) -> None:
    """The table died: drop its entry (if it is still the relation's)."""
    csr, entry = csr_ref(), entry_ref()
    if csr is not None and entry is not None and csr.__dict__.get("_static_agg") is entry:
        del csr.__dict__["_static_agg"]
        _STATIC_HOLDERS.discard(csr)


def _static_lookup(x: torch.Tensor, csr: RelationCSR, blocks: int, name: Optional[str],
                   fingerprint=table_fingerprint) -> Optional[torch.Tensor]:
    """The kept aggregate of ``x`` over ``csr``, or None: a hit needs the same live tensor
    object at the same pointer, shape, strides and version."""
    entry = csr.__dict__.get("_static_agg")
    if entry is None:
        return None
    if entry.ref() is not x or entry.key != _static_key(x, blocks):
        return None
    if STATIC_AGG == "check":
        if entry.fp is None:          # kept before the check was switched on: recompute
            return None
        if int(fingerprint(x)) != int(entry.fp):   # (a host sync per hit)
            what = name or f"{csr.n_src}->{csr.n_dst} rows"
            raise StaleAggregateError(
                f"static aggregate of relation {what} ({csr.num_edges} edges): the source "
                "table's memory changed without a version bump (a kernel wrote it through a raw "
                "pointer?) — call ops.clear_static_aggregates() after such a write")
    if entry.event is not None:
        cur = torch.cuda.current_stream(entry.value.device)
        if cur != entry.stream:
            cur.wait_event(entry.event)
    return entry.value


def _static_store(x: torch.Tensor, csr: RelationCSR, blocks: int, value: torch.Tensor,
                  fingerprint=table_fingerprint) -> None:
    """Keep ``value`` as the aggregate of ``x`` over ``csr`` (replacing the relation's entry)."""
    fp = fingerprint(x) if STATIC_AGG == "check" else None
    old = csr.__dict__.get("_static_agg")
    if old is not None and old.fin is not None:
        old.fin.detach()      # (a table changed in place every step leaves no finalizers behind)
    entry = _StaticEntry(x, _static_key(x, blocks), value, fp)
    csr.__dict__["_static_agg"] = entry
    _STATIC_HOLDERS.add(csr)
    entry.fin = weakref.finalize(x, _static_drop, weakref.ref(csr), weakref.ref(entry))


def _static_aggregate(x: torch.Tensor, csr: RelationCSR, blocks: int, name: Optional[str],
                      compute, fingerprint=table_fingerprint) -> torch.Tensor:
    """``compute()`` once per (table, relation): the kept result on a hit, else computed and kept
    (``compute`` / ``fingerprint`` are parameters so the keying is testable without a GPU)."""
    if not _static_enabled(x):
        return compute()
    kept = _static_lookup(x, csr, blocks, name, fingerprint)
    if kept is None:
        kept = compute()
        _static_store(x, csr, blocks, kept, fingerprint)
    return kept


def clear_static_aggregates() -> None:
    """Drop every kept static aggregate.  Whoever rewrites an input table through a raw pointer
    (a native kernel writing into it or into a view of it: no version bump) must call this."""
    for csr in list(_STATIC_HOLDERS):
        csr.__dict__.pop("_static_agg", None)
    _STATIC_HOLDERS.clear()


def static_aggregate_count() -> int:
    """Number of kept static aggregates (live relations holding one)."""
    return sum(1 for csr in list(_STATIC_HOLDERS) if "_static_agg" in csr.__dict__)


def gather_mean(x_src: torch.Tensor, csr: RelationCSR,
                out: Optional[torch.Tensor] = None, static: bool = False,
                name: Optional[str] = None) -> torch.Tensor:
    """K1: ``aggr[i] = mean_{(j->i)} x_src[j]`` (0 for an empty row); added into ``out`` when
    given.

    ``static=True``: the caller declares ``x_src`` a static model input (never a layer output,
    never a sampled block's buffer).  The aggregate is then computed once by this same call and
    kept on ``csr`` for as long as ``x_src`` lives unchanged: the key holds the tensor weakly with
    its ``data_ptr()``, shape, strides and ``_version``, so an in-place torch op, a new tensor or
    the table's death all miss.  The returned tensor is shared between calls and MUST NOT be
    written.  A write to the table that bypasses torch (a native kernel through a raw pointer)
    bumps no version: whoever does that must call :func:`clear_static_aggregates`
    (``HGNN_STATIC_AGG=check`` verifies a checksum of the table on every hit and raises
    :class:`StaleAggregateError`, naming the relation by ``name``).  ``HGNN_STATIC_AGG=0`` turns
    the keeping off."""
    if static and out is not None:
        raise ValueError("gather_mean: a static aggregate is never accumulated into (out=)")
    if static and x_src.dtype == torch.bfloat16:
        raise ValueError("gather_mean: a static model input is gathered once and kept as fp32 "
                         "rows; bf16 rows are for tables that change every step (static=True "
                         "with a bfloat16 table)")
    given = x_src
    x_src = _check_table(x_src, "gather_mean")
    dev = N.require_device(x_src, csr.fwd.rowptr)
    if x_src.shape[0] != csr.n_src:
        raise ValueError(f"x_src has {x_src.shape[0]} rows, relation expects {csr.n_src}")
    if static and x_src is given and not x_src.requires_grad:
        B = gather_blocks(x_src, csr.num_edges) if csr.num_edges else 1
        return _static_aggregate(x_src, csr, B, name, lambda: gather_mean(x_src, csr))
    d = int(x_src.shape[1])
    acc = out is not None
    if out is None:
        out = torch.empty(csr.n_dst, d, dtype=torch.float32, device=dev)
    B = gather_blocks(x_src, csr.num_edges) if csr.num_edges else 1
    if B > 1:
        passes, _ = csr.blocks("fwd", B)
        E = csr.num_edges
        rb = _row_bytes(x_src)
        _gather_blocked(x_src, passes, csr.inv_deg, None, out, acc,
                        f"gather_fwd[{csr.n_dst}<-{csr.n_src}]x{d}",
                        gather_bytes(E, csr.n_dst, d, False, rb),
                        gather_compulsory_bytes(E, csr.n_dst, csr.n_src, d, False, rb))
        return out
    _gather(x_src, csr.fwd, None, csr_mean=True, out=out, accumulate=acc,
            hot=csr.hot_cols("fwd", _table_bytes(x_src)))
    return out


def _multi_ok(jobs) -> bool:
    """Whether gathers (x, grouped, out) can share one ``hgnn_gather_reduce_multi`` launch:
    2..8 of them, no heavy-row plan, one fp32 row width (a multiple of 4, <= 512), distinct
    outputs, and no per-kernel timer running (its events time each relation's launch)."""
    if _timer is not None or not 2 <= len(jobs) <= 8:
        return False
    d = int(jobs[0][2].shape[1])
    outs = {o.data_ptr() for _, _, o in jobs}
    return (len(outs) == len(jobs) and d % 4 == 0 and d <= 512 and
            all(g.plan.n_heavy == 0 and int(o.shape[1]) == d and x.dtype == torch.float32
                for x, g, o in jobs))


def _gather_multi(jobs, mean: bool, accumulate: bool, edge_ws=None, acc_limit=None) -> None:
    """``_gather`` of every (x, grouped, out) job in one launch (see ``_multi_ok``);
    ``acc_limit[j]`` > 0: job j accumulates only into its rows below it."""
    dev = jobs[0][2].device
    flags = (N.HGNN_MEAN if mean else 0) | (N.HGNN_ACCUMULATE if accumulate else 0)
    N.check(N.lib().hgnn_gather_reduce_multi(
        len(jobs), N.ptr_array([x for x, _, _ in jobs]),
        N.i64_array([int(x.shape[0]) for x, _, _ in jobs]), int(jobs[0][2].shape[1]),
        N.ptr_array([g.rowptr for _, g, _ in jobs]), N.ptr_array([g.col for _, g, _ in jobs]),
        N.i64_array([g.n_rows for _, g, _ in jobs]),
        N.ptr_array(edge_ws) if edge_ws is not None else None, flags,
        N.i64_array(acc_limit) if acc_limit is not None else None,
        N.ptr_array([o for _, _, o in jobs]), N.stream_ptr(dev)), "hgnn_gather_reduce_multi")


def gather_mean_many(pairs: Sequence[Tuple[torch.Tensor, RelationCSR]],
                     static: Sequence[bool] = (), names: Sequence[Optional[str]] = ()
                     ) -> List[torch.Tensor]:
    """``gather_mean(x, csr)`` of every pair — one launch for all of them when they qualify
    (sampled blocks: short rows, one pass each; ``_multi_ok``), else one call each.
    ``static[i]``: pair i's table is a static model input (see :func:`gather_mean`); such pairs
    go through the kept aggregates one by one and only the rest are launched here."""
    if any(static) and STATIC_AGG != "0":
        res: List[Optional[torch.Tensor]] = [None] * len(pairs)
        rest = []
        for i, (x, csr) in enumerate(pairs):
            if i < len(static) and static[i]:
                res[i] = gather_mean(x, csr, static=True,
                                     name=names[i] if i < len(names) else None)
            else:
                rest.append(i)
        if rest:
            for i, o in zip(rest, gather_mean_many([pairs[i] for i in rest])):
                res[i] = o
        return res
    jobs = []
    for x, csr in pairs:
        x = _check_f32(x, "gather_mean")
        if x.shape[0] != csr.n_src:
            raise ValueError(f"x_src has {x.shape[0]} rows, relation expects {csr.n_src}")
        if csr.num_edges and gather_blocks(x, csr.num_edges) > 1:
            return [gather_mean(x, c) for x, c in pairs]
        jobs.append((x, csr.fwd, torch.empty(csr.n_dst, int(x.shape[1]), dtype=torch.float32,
                                             device=x.device)))
    if not _multi_ok(jobs):
        return [gather_mean(x, c) for x, c in pairs]
    _gather_multi(jobs, mean=True, accumulate=False)
    return [o for _, _, o in jobs]


# ----------------------------------------------------------------------------- zero-packed rows
# A K3 output that went through the fused ReLU carries this attribute (set True where such
# outputs are produced, ``linear_fwd`` / ``linear_fwd_many``).  It is a hint about sparsity and
# nothing else: the packed format is lossless (``csrc/zpack.h``), so a stale mark on a tensor
# somebody wrote into afterwards costs time, never a wrong result.
RELU_OUT = "_hgnn_relu_out"


def zpack_on(x: torch.Tensor, relu_out: bool) -> bool:
    """Whether the loss's dP gather reads ``x`` zero-packed: ``HGNN_ZPACK`` = ``0`` never, ``1``
    whenever the width is 64 or 128, ``auto`` (the default) for a fused-ReLU K3 output of at
    least 1 GiB with such a width (``hgnn_zpack_policy``, read per call)."""
    return bool(N.lib().hgnn_zpack_policy(_table_bytes(x), int(x.shape[1]), 1 if relu_out else 0))


def zpack_rows(x: torch.Tensor, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The zero-packed copy of an fp32 table of width 64 or 128 (``hgnn_zpack_rows``): a uint8
    tensor of ``n * hgnn_zpack_slot_bytes(d)`` bytes, per row a 16-B mask and the non-zero bit
    patterns; the rest of each slot stays unwritten.  ``hist`` (6 int64 counters on the device)
    has the rows counted into it by the 128-B lines they take."""
    x = _check_f32(x, "zpack_rows")
    dev = N.require_device(x)
    n, d = int(x.shape[0]), int(x.shape[1])
    slot = int(N.lib().hgnn_zpack_slot_bytes(d))
    if slot == 0:
        raise ValueError(f"zpack_rows: d={d}; zero-packed rows are 64 or 128 wide")
    out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    # (bytes: the table read and, the sparsity unknown here, mask + every value written)
    with _timed(f"zpack[{n}]x{d}", n * (4 * d + 16 + 4 * d)):
        N.check(N.lib().hgnn_zpack_rows(N.ptr(x), n, d, N.ptr(out), N.ptr(hist),
                                        N.stream_ptr(dev)), "hgnn_zpack_rows")
    return out


def _table_bytes(x: torch.Tensor) -> int:
    return x.numel() * x.element_size()


def _gather(x, grouped, col_w, csr_mean, out, accumulate, edge_w=None, kind=None, hot=None):
    """``hot``: the grouping's ``graph.HotCols`` (``RelationCSR.hot_cols``) or None; with one the
    launch goes through ``hgnn_gather_reduce_hot`` (two-policy row loads, same sums)."""
    flags = (N.HGNN_MEAN if csr_mean else 0) | (N.HGNN_ACCUMULATE if accumulate else 0)
    d = int(out.shape[1])
    weighted = edge_w is not None or col_w is not None
    kind = kind or ("fwd" if csr_mean else "bwd")   # "wfwd": weighted forward (parallel.py)
    name = f"gather_{kind}[{grouped.n_rows}<-{x.shape[0]}]x{d}"   # [dst rows <- src rows] x d
    E = int(grouped.col.numel())
    rb = _row_bytes(x)
    with _timed(name, gather_bytes(E, grouped.n_rows, d, weighted, rb),
                gather_compulsory_bytes(E, grouped.n_rows, int(x.shape[0]), d, weighted, rb)):
        _launch_gather(x, grouped, edge_w, col_w, None, flags, out, hot)


def _score_gather(U, P, grouped, mode, cscale, inv_e, out, accumulate, tag):
    """dP rows from the loss: each edge's weight recomputed from <U[u], P[row]> (mode 1 positive,
    2 negative) inside the gather — see hgnn_score_gather."""
    dev = out.device
    d = int(out.shape[1])
    plan = _plan_args(grouped.plan, d, dev)
    E = int(grouped.col.numel())
    nb = gather_bytes(E, grouped.n_rows, d, False) + 4 * grouped.n_rows * d
    cb = (gather_compulsory_bytes(E, grouped.n_rows, int(U.shape[0]), d, False)
          + 4 * grouped.n_rows * d)
    with _timed(f"score_gather_{tag}[{grouped.n_rows}<-{U.shape[0]}]x{d}", nb, cb):
        N.check(N.lib().hgnn_score_gather(
            N.ptr(U), U.shape[0], N.ptr(P), d, N.ptr(grouped.rowptr), N.ptr(grouped.col),
            grouped.n_rows, mode, N.ptr(cscale), inv_e, *plan, N.ptr(out),
            1 if accumulate else 0, N.stream_ptr(dev)), "hgnn_score_gather")


class _NegPlan(NamedTuple):
    """The heavy-row plan of one step's negatives' lists, on the device (``hgnn_plan_device``):
    arrays sized by the bound ``max_heavy = pairs // chunk``, the counts never read back."""
    heavy_rows: torch.Tensor      # int32 [max(max_heavy, 1)]
    heavy_first: torch.Tensor     # int32 [max_heavy + 1]
    counts: torch.Tensor          # int32 [2]: n_heavy, n_chunks
    max_heavy: int
    chunk: int


def _plan_negatives(rowptr_n: torch.Tensor, n_posts: int, n_pairs: int, chunk: int) -> _NegPlan:
    """The plan of the negatives' lists ``rowptr_n`` (``n_pairs`` entries over ``n_posts`` rows)
    for the chunk of the positives' plan.  A list is heavy above ``chunk`` entries, so at most
    ``n_pairs // chunk`` lists are, and they have at most twice that many chunks."""
    dev = rowptr_n.device
    lib = N.lib()
    max_heavy = n_pairs // chunk
    heavy_rows = torch.empty(max(max_heavy, 1), dtype=torch.int32, device=dev)
    heavy_first = torch.empty(max_heavy + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ws = N.workspace(lib.hgnn_plan_ws_bytes(n_posts), dev)
    with _timed("plan_negatives", 4 * n_posts * 10):
        N.check(lib.hgnn_plan_device(N.ptr(rowptr_n), n_posts, chunk, max_heavy,
                                     N.ptr(heavy_rows), N.ptr(heavy_first), N.ptr(counts),
                                     N.ptr(ws), ws.numel(), N.stream_ptr(dev)),
                "hgnn_plan_device")
    return _NegPlan(heavy_rows, heavy_first, counts, max_heavy, chunk)


def _score_gather2_planned(U, P, pos, negs, cscale, inv_e, out, Uz, edge_w, plan: _NegPlan,
                           pplan: _PlanArgs, nb, cb, row_bias=None):
    """``_score_gather2`` through ``hgnn_score_gather2_planned``: the negatives' heavy lists go
    chunk by chunk into a slab of their own, ``2 * max_heavy`` rows of d floats (the bound on the
    chunks; at 200M pairs, chunk 1024 and d = 128 that is 200 MB), allocated per call.
    ``row_bias``: ``hgnn_score_gather2_planned_lq``."""
    dev = out.device
    d = int(out.shape[1])
    n = pos.n_rows
    if plan.chunk != pos.plan.chunk:
        raise ValueError("edge_bce_loss: the negatives' plan was made for another chunk")
    rows, table = ((1, U) if U.dtype == torch.bfloat16 else (2, Uz) if Uz is not None else (0, U))
    neg_slab = torch.empty(max(2 * plan.max_heavy, 1) * d, dtype=torch.float32, device=dev)
    entry = "hgnn_score_gather2_planned" + ("_lq" if row_bias is not None else "")
    bias = (N.ptr(row_bias),) if row_bias is not None else ()
    with _timed(f"score_gather_planned[{n}<-{U.shape[0]}]x{d}", nb, cb):
        N.check(getattr(N.lib(), entry)(
            rows, N.ptr(table), U.shape[0], N.ptr(P), d, N.ptr(pos.rowptr), N.ptr(pos.col),
            N.ptr(edge_w), N.ptr(negs.rowptr), N.ptr(negs.col), n, N.ptr(cscale), inv_e, *bias,
            *pplan, N.ptr(plan.heavy_rows), N.ptr(plan.heavy_first), N.ptr(plan.counts),
            plan.max_heavy, N.ptr(neg_slab), N.ptr(out), N.stream_ptr(dev)), entry)


def _score_gather2(U, P, pos, negs, cscale, inv_e, out, Uz=None, edge_w=None, neg_plan=None,
                   row_bias=None):
    """Both dP gathers in one pass (hgnn_score_gather2): row r sums its positive edges (mode 1,
    heavy-row plan) and its negatives (mode 2) into one accumulator and writes dP[r] once.
    ``Uz``: ``zpack_rows(U)``; the gather then reads the packed rows (same sums, bit for bit;
    the timer entry keeps its name and the unpacked table's algorithmic bytes).  ``edge_w``: the
    positives' per-edge weights by position of ``pos`` (the ``_w`` entries; 4 B more per
    positive edge).  ``neg_plan``: the ``_NegPlan`` of ``SkewedNegatives``; the gather is then
    ``hgnn_score_gather2_planned``.  ``row_bias``: the logQ table (fp32 ``[n]``): the ``_lq``
    entries, each row's offset subtracted from its scores (4 B more per output row)."""
    dev = out.device
    d = int(out.shape[1])
    n = pos.n_rows
    plan = _plan_args(pos.plan, d, dev)
    E = int(pos.col.numel()) + int(negs.col.numel())
    rb = _row_bytes(U)      # U's rows per edge and P's own row per output row
    wb = 4 * int(pos.col.numel()) if edge_w is not None else 0
    wb += 4 * n if row_bias is not None else 0
    nb = gather_bytes(E, n, d, False, rb) + 4 * (n + 1) + n * rb + wb
    cb = gather_compulsory_bytes(E, n, int(U.shape[0]), d, False, rb) + 4 * (n + 1) + n * rb + wb
    if neg_plan is not None:
        _score_gather2_planned(U, P, pos, negs, cscale, inv_e, out, Uz, edge_w, neg_plan, plan,
                               nb, cb, row_bias)
        return
    if row_bias is not None:   # one entry for the three row formats, edge_w nullable
        fmt, table = ((1, U) if U.dtype == torch.bfloat16 else (2, Uz) if Uz is not None else (0, U))
        with _timed(f"score_gather[{n}<-{U.shape[0]}]x{d}", nb, cb):
            N.check(N.lib().hgnn_score_gather2_lq(
                fmt, N.ptr(table), U.shape[0], N.ptr(P), d, N.ptr(pos.rowptr), N.ptr(pos.col),
                N.ptr(edge_w), N.ptr(negs.rowptr), N.ptr(negs.col), n, N.ptr(cscale), inv_e,
                N.ptr(row_bias), *plan, N.ptr(out), N.stream_ptr(dev)), "hgnn_score_gather2_lq")
        return
    # the entry point by the rows it reads: bf16, zero-packed fp32, fp32
    rows, table = (("_bf16", U) if U.dtype == torch.bfloat16 else
                   ("_zp", Uz) if Uz is not None else ("", U))
    entry = "hgnn_score_gather2" + ("_w" if edge_w is not None else "") + rows
    weights = (N.ptr(edge_w),) if edge_w is not None else ()
    with _timed(f"score_gather[{n}<-{U.shape[0]}]x{d}", nb, cb):
        N.check(getattr(N.lib(), entry)(
            N.ptr(table), U.shape[0], N.ptr(P), d, N.ptr(pos.rowptr), N.ptr(pos.col), *weights,
            N.ptr(negs.rowptr), N.ptr(negs.col), n, N.ptr(cscale), inv_e, *plan, N.ptr(out),
            N.stream_ptr(dev)), entry)


def scatter_mean_bwd(grad_aggr: torch.Tensor, csr: RelationCSR,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K2: ``grad_x_src[j] (+)= sum_{(j->i)} grad_aggr[i] / deg_i`` over the CSC.  ``grad_aggr``:
    fp32, or the bf16 gradient rows of ``grad_row_dtype`` (sums and ``out`` stay fp32)."""
    grad_aggr = _check_table(grad_aggr, "scatter_mean_bwd")
    dev = grad_aggr.device
    d = int(grad_aggr.shape[1])
    acc = out is not None
    if out is None:
        out = torch.empty(csr.n_src, d, dtype=torch.float32, device=dev)
    B = gather_blocks(grad_aggr, csr.num_edges) if csr.num_edges else 1
    if B > 1:
        passes, w = csr.blocks("bwd", B)
        E = csr.num_edges
        rb = _row_bytes(grad_aggr)
        _gather_blocked(grad_aggr, passes, None, w, out, acc,
                        f"gather_bwd[{csr.n_src}<-{csr.n_dst}]x{d}",
                        gather_bytes(E, csr.n_src, d, True, rb),
                        gather_compulsory_bytes(E, csr.n_src, csr.n_dst, d, True, rb))
        return out
    _gather(grad_aggr, csr.bwd, None, csr_mean=False, out=out, accumulate=acc,
            edge_w=csr.bwd_weights, hot=csr.hot_cols("bwd", _table_bytes(grad_aggr)))
    return out


def relu_mask_for(n: int, h: int, relu: bool, dev, k: Optional[int] = None
                  ) -> Optional[torch.Tensor]:
    """The bit form of a K3 output's ReLU mask (``hgnn_linear_fwd_mask``: 16 B per row, the
    backward reads it instead of the 4h-byte output), or None where the kernels have no bit form
    (no ReLU, h not a multiple of 16 or above 128) or where no kernel would read it: an input
    width ``k`` outside the persistent kernels' {64, 128, 256} (the general kernels read the
    output, and the bits would cost a separate launch)."""
    if not (relu and h % 16 == 0 and h <= 128):
        return None
    if k is not None and k not in (64, 128, 256):
        return None
    return torch.empty((n, 4), dtype=torch.int32, device=dev)


def _check_rows(segs, n, what):
    """Every segment of a K3 call has the same n rows (the kernels read each without bounds)."""
    for i, s_ in enumerate(segs):
        if s_.dim() != 2 or int(s_.shape[0]) != n:
            raise ValueError(f"{what}: segment {i} is {tuple(s_.shape)}, expected {n} rows")


def _lin_fwd_job(what, segs, w, b, add=None, mask_out=None):
    """One K3 forward's shape checks (errors named after the caller, ``what``), its output buffer
    and its traffic / flop counts for the kernel timer: ``(n, h, ks, out, nbytes, flops)``."""
    n = int(segs[0].shape[0])
    h = int(w.shape[0])
    ks = [int(s.shape[1]) for s in segs]
    k = sum(ks)
    if w.shape[1] != k:
        raise ValueError(f"weight has {w.shape[1]} input columns, segments sum to {k}")
    _check_rows(segs, n, what)
    if add is not None and tuple(add.shape) != (n, h):
        raise ValueError(f"{what}: add is {tuple(add.shape)}, expected {(n, h)}")
    if b is not None and b.numel() != h:
        raise ValueError(f"{what}: bias has {b.numel()} entries, expected {h}")
    out = torch.empty(n, h, dtype=torch.float32, device=w.device)
    nb = 4 * n * (k + h + (h if add is not None else 0)) + (16 * n if mask_out is not None else 0)
    return n, h, ks, out, nb, 2 * n * k * h


def linear_fwd(segs: Sequence[torch.Tensor], w: torch.Tensor, b: Optional[torch.Tensor],
               relu: bool, add: Optional[torch.Tensor] = None,
               mask_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3/K4: ``act(sum_s segs[s] @ w[:, seg s]^T + b (+ add))``; ``mask_out`` (from
    :func:`relu_mask_for`) also receives the ReLU mask as bits."""
    n, h, ks, out, nb, fl = _lin_fwd_job("linear_fwd", segs, w, b, add, mask_out)
    with _timed(f"linear_fwd[{n}x{sum(ks)}->{h}]", nb, flops=fl):
        N.check(N.lib().hgnn_linear_fwd_mask(len(segs), N.ptr_array(segs), N.int_array(ks), n,
                                             N.ptr(w), h, N.ptr(b), N.ptr(add),
                                             1 if relu else 0, N.ptr(out), N.ptr(mask_out),
                                             N.stream_ptr(w.device)), "hgnn_linear_fwd_mask")
    if relu:
        setattr(out, RELU_OUT, True)
    return out


def _lin_bwd_job(what, segs, w, dout, out_act, dxs, need_w, need_b, dz_out=None, mask=None,
                 dx_add=()):
    """One K3 backward's shape checks (errors named after the caller, ``what``), its weight
    gradient buffers, its accumulate bits and its traffic / flop counts for the kernel timer:
    ``(n, h, ks, dw, db, acc, nbytes, flops)``."""
    n = int(segs[0].shape[0])
    h = int(w.shape[0])
    ks = [int(s.shape[1]) for s in segs]
    k = sum(ks)
    if w.shape[1] != k:
        raise ValueError(f"weight has {w.shape[1]} input columns, segments sum to {k}")
    _check_rows(segs, n, what)
    for name, t in (("dout", dout), ("out_act", out_act), ("dz_out", dz_out)):
        if t is not None and tuple(t.shape) != (n, h):
            raise ValueError(f"{what}: {name} is {tuple(t.shape)}, expected {(n, h)}")
    if len(dxs) != len(segs):
        raise ValueError(f"{what}: {len(dxs)} dx buffers for {len(segs)} segments")
    for s_, dx in zip(segs, dxs):
        if dx is not None and tuple(dx.shape) != tuple(s_.shape):
            raise ValueError(f"{what}: dx {tuple(dx.shape)} for a {tuple(s_.shape)} segment")
    if mask is not None and tuple(mask.shape) != (n, 4):
        raise ValueError(f"{what}: ReLU bits are {tuple(mask.shape)}, expected {(n, 4)}")
    dw = torch.empty_like(w) if need_w else None
    db = torch.empty(h, dtype=torch.float32, device=w.device) if need_b else None
    k_dx = sum(kk for kk, dx in zip(ks, dxs) if dx is not None)
    bits = mask is not None and out_act is not None
    nb = 4 * n * (h + (h if out_act is not None and not bits else 0) + k + k_dx) + \
        (16 * n if bits else 0) + (4 * n * h if dz_out is not None else 0)
    fl = 2 * n * h * k_dx + (2 * n * k * h if need_w else 0)   # dgrad + wgrad
    acc = 0
    for i, on in enumerate(dx_add):
        if on and dxs[i] is not None:
            acc |= 1 << i
            nb += 4 * n * ks[i]          # the gradient already there is read back
    return n, h, ks, dw, db, acc, nb, fl


def linear_bwd(segs, w, dout, out_act, dxs: Sequence[Optional[torch.Tensor]], need_w: bool,
               need_b: bool, dz_out: Optional[torch.Tensor] = None,
               mask: Optional[torch.Tensor] = None, dx_add: Sequence[bool] = ()):
    """K3 backward; ``dz_out`` (optional [n, h]) receives the masked dz as well; ``mask``: the
    forward's ReLU bits (read instead of ``out_act`` by the persistent kernels); ``dx_add[s]``:
    segment s's input gradient is added into what ``dxs[s]`` holds (``hgnn_linear_bwd_ex``)."""
    n, h, ks, dw, db, acc, nb, fl = _lin_bwd_job("linear_bwd", segs, w, dout, out_act, dxs,
                                                 need_w, need_b, dz_out, mask, dx_add)
    dev = w.device
    ws = None
    if need_w or need_b:
        ws = N.workspace(N.lib().hgnn_linear_bwd_ws_bytes(n, sum(ks), h), dev)
    with _timed(f"linear_bwd[{n}x{sum(ks)}->{h}]", nb, flops=fl):
        N.check(N.lib().hgnn_linear_bwd_ex(
            len(segs), N.ptr_array(segs), N.int_array(ks), n, N.ptr(w), h, N.ptr(dout),
            N.ptr(out_act), N.ptr(mask if out_act is not None else None), N.ptr_array(dxs),
            acc, N.ptr(dw), N.ptr(db), N.ptr(dz_out), N.ptr(ws), 0 if ws is None else ws.numel(),
            N.stream_ptr(dev)), "hgnn_linear_bwd_ex")
    return dw, db


class FwdJob(NamedTuple):
    """One K3 forward of :func:`linear_fwd_many`."""
    segs: Sequence[torch.Tensor]
    w: torch.Tensor
    b: Optional[torch.Tensor]
    relu: bool
    mask: Optional[torch.Tensor]          # relu_mask_for's buffer: receives the ReLU bits


class BwdJob(NamedTuple):
    """One K3 backward of :func:`linear_bwd_many`."""
    segs: Sequence[torch.Tensor]
    w: torch.Tensor
    dout: torch.Tensor
    out_act: Optional[torch.Tensor]       # the forward's output where it went through a ReLU
    dxs: Sequence[Optional[torch.Tensor]]
    need_w: bool
    need_b: bool
    mask: Optional[torch.Tensor]          # the forward's ReLU bits


def linear_fwd_many(jobs) -> List[torch.Tensor]:
    """:func:`linear_fwd` (no ``add``) of each :class:`FwdJob` (or plain tuple in its field
    order) in one native call (``hgnn_linear_fwd_multi``): a sampled layer's two destination
    types on the K = 384 / 512 split path share each column block's launch; anything else runs
    job by job there."""
    jobs = [FwdJob(*j) for j in jobs]
    if len(jobs) == 1 or len({int(j.w.shape[0]) for j in jobs}) > 1:   # (one output width)
        return [linear_fwd(j.segs, j.w, j.b, j.relu, mask_out=j.mask) for j in jobs]
    info = [_lin_fwd_job("linear_fwd_many", j.segs, j.w, j.b, mask_out=j.mask) for j in jobs]
    rows, outs = [i[0] for i in info], [i[3] for i in info]
    ks = [k for i in info for k in i[2]]
    dev, h = jobs[0].w.device, info[0][1]
    with _timed(f"linear_fwd_multi[{'+'.join(str(r) for r in rows)}x{sum(ks) // len(jobs)}->{h}]",
                sum(i[4] for i in info), flops=sum(i[5] for i in info)):
        N.check(N.lib().hgnn_linear_fwd_multi(
            len(jobs), N.int_array([len(j.segs) for j in jobs]),
            N.ptr_array([s_ for j in jobs for s_ in j.segs]), N.int_array(ks), N.i64_array(rows),
            N.ptr_array([j.w for j in jobs]), h, N.ptr_array([j.b for j in jobs]),
            N.int_array([1 if j.relu else 0 for j in jobs]), N.ptr_array(outs),
            N.ptr_array([j.mask for j in jobs]), N.stream_ptr(dev)), "hgnn_linear_fwd_multi")
    for j, o in zip(jobs, outs):
        if j.relu:
            setattr(o, RELU_OUT, True)
    return outs


def _linear_bwd_of(j: BwdJob):
    """:func:`linear_bwd` of one job."""
    return linear_bwd(j.segs, j.w, j.dout, j.out_act, j.dxs, j.need_w, j.need_b, mask=j.mask)


def linear_bwd_many(jobs):
    """:func:`linear_bwd` (no ``dz_out``, no ``dx_add``) of each :class:`BwdJob` (or plain tuple
    in its field order) in one native call (``hgnn_linear_bwd_multi``); returns the ``(dw, db)``
    of each."""
    jobs = [BwdJob(*j) for j in jobs]
    if len(jobs) == 1 or len({int(j.w.shape[0]) for j in jobs}) > 1:
        return [_linear_bwd_of(j) for j in jobs]
    info = [_lin_bwd_job("linear_bwd_many", j.segs, j.w, j.dout, j.out_act, j.dxs, j.need_w,
                         j.need_b, mask=j.mask) for j in jobs]
    rows, kt = [i[0] for i in info], [sum(i[2]) for i in info]
    dws, dbs = [i[3] for i in info], [i[4] for i in info]
    dev, h = jobs[0].w.device, info[0][1]
    ws = None
    if any(d is not None for d in dws + dbs):
        ws = N.workspace(N.lib().hgnn_linear_bwd_multi_ws_bytes(
            len(jobs), N.i64_array(rows), N.int_array(kt), h), dev)
    with _timed(f"linear_bwd_multi[{'+'.join(str(r) for r in rows)}x{sum(kt) // len(jobs)}->{h}]",
                sum(i[6] for i in info), flops=sum(i[7] for i in info)):
        N.check(N.lib().hgnn_linear_bwd_multi(
            len(jobs), N.int_array([len(j.segs) for j in jobs]),
            N.ptr_array([s_ for j in jobs for s_ in j.segs]),
            N.int_array([k for i in info for k in i[2]]), N.i64_array(rows),
            N.ptr_array([j.w for j in jobs]), h, N.ptr_array([j.dout for j in jobs]),
            N.ptr_array([j.out_act for j in jobs]),
            N.ptr_array([j.mask if j.out_act is not None else None for j in jobs]),
            N.ptr_array([d for j in jobs for d in j.dxs]), None, N.ptr_array(dws),
            N.ptr_array(dbs), N.ptr(ws), 0 if ws is None else ws.numel(), N.stream_ptr(dev)),
            "hgnn_linear_bwd_multi")
    return list(zip(dws, dbs))


# ----------------------------------------------------------------------------- fused weights
def split_weight_grads(dW: torch.Tensor, db: Optional[torch.Tensor], ks: Sequence[int],
                       k_root: int, scales: Sequence[float],
                       dwl: Sequence[Optional[torch.Tensor]], dwr: Sequence[Optional[torch.Tensor]],
                       dbl: Sequence[Optional[torch.Tensor]], plan=None) -> None:
    """Adjoint of :func:`fuse_weights` into the given gradient buffers (entries may be None):
    dwl[r] = s_r dW[:, block r], dwr[r] = s_r dW[:, root], dbl[r] = s_r db (one launch)."""
    dev = dW.device
    a_ks = plan.a_ks if plan is not None else N.int_array(ks)
    a_sc = plan.a_sc if plan is not None else N.float_array(scales)
    N.check(N.lib().hgnn_split_weight_grads(
        len(ks), N.ptr(dW.contiguous()), N.ptr(None if db is None else db.contiguous()),
        a_ks, int(k_root), a_sc, int(dW.shape[0]),
        N.ptr_array(dwl), N.ptr_array(dwr), N.ptr_array(dbl), N.stream_ptr(dev)),
        "hgnn_split_weight_grads")


class _FusePlan:
    """The host side of one fused-weight launch, built once per set of parameter buffers: the
    layout (meta) and the ctypes argument arrays.  Parameters keep their storage across
    optimizer steps, so a sampled mini-batch step (four of these per step at cfg5, where the
    host issue time is the step time) reuses them instead of rebuilding them per call."""
    __slots__ = ("meta", "a_wl", "a_wr", "a_bl", "a_ks", "a_sc")

    def __init__(self, meta, wl, wr, bl):
        ks, k_root, scales, _, _ = meta
        self.meta = meta
        self.a_wl, self.a_wr, self.a_bl = N.ptr_array(wl), N.ptr_array(wr), N.ptr_array(bl)
        self.a_ks, self.a_sc = N.int_array(ks), N.float_array(scales)


_FUSE_PLANS: "Dict[tuple, _FusePlan]" = {}


def _fuse_plan(meta, wl, wr, bl) -> _FusePlan:
    ts = [t for t in (*wl, *wr, *bl) if t is not None]
    if not all(t.is_contiguous() for t in ts):
        return _FusePlan(meta, [t.contiguous() for t in wl],
                         [None if t is None else t.contiguous() for t in wr],
                         [None if t is None else t.contiguous() for t in bl])
    key = (meta, tuple(0 if t is None else t.data_ptr() for t in (*wl, *wr, *bl)))
    plan = _FUSE_PLANS.get(key)
    if plan is None:
        if len(_FUSE_PLANS) >= 1024:
            _FUSE_PLANS.clear()
        plan = _FUSE_PLANS[key] = _FusePlan(meta, wl, wr, bl)
    return plan


class _FuseWeights(torch.autograd.Function):
    """``[s_1 Wl_1 | ... | s_R Wl_R | sum_r s_r Wr_r]`` and ``sum_r s_r bl_r`` in one launch
    (``hgnn_fuse_weights``); backward: every parameter's gradient in one launch."""

    @staticmethod
    def forward(ctx, meta, *ts):
        ks, k_root, scales, has_r, has_b = meta
        R = len(ks)
        wl, it = list(ts[:R]), iter(ts[R:])
        wr = [next(it) if hr else None for hr in has_r]
        bl = [next(it) if hb else None for hb in has_b]
        h, dev = int(wl[0].shape[0]), wl[0].device
        W = torch.empty(h, sum(ks) + k_root, dtype=torch.float32, device=dev)
        b = torch.empty(h, dtype=torch.float32, device=dev) if any(has_b) else None
        plan = _fuse_plan(meta, wl, wr, bl)
        N.check(N.lib().hgnn_fuse_weights(R, plan.a_wl, plan.a_ks, plan.a_wr, int(k_root),
                                          plan.a_bl, plan.a_sc, h, N.ptr(W), N.ptr(b),
                                          N.stream_ptr(dev)), "hgnn_fuse_weights")
        ctx.meta, ctx.h, ctx.dev, ctx.plan = meta, h, dev, plan
        return (W, b) if b is not None else W

    @staticmethod
    def backward(ctx, dW, db=None):
        ks, k_root, scales, has_r, has_b = ctx.meta
        R = len(ks)
        need = ctx.needs_input_grad[1:]
        new = lambda shape, i: (torch.empty(shape, dtype=torch.float32, device=ctx.dev)
                                if need[i] else None)
        dwl = [new((ctx.h, k), r) for r, k in enumerate(ks)]
        i = R
        dwr, dbl = [], []
        for hr in has_r:
            dwr.append(new((ctx.h, k_root), i) if hr else None)
            i += hr
        for hb in has_b:
            dbl.append(new((ctx.h,), i) if hb else None)
            i += hb
        if dW is None:
            dW = torch.zeros(ctx.h, sum(ks) + k_root, dtype=torch.float32, device=ctx.dev)
        split_weight_grads(dW, db if any(has_b) else None, ks, k_root, scales, dwl, dwr, dbl,
                           plan=ctx.plan)
        return (None, *dwl, *[t for t, hr in zip(dwr, has_r) if hr],
                *[t for t, hb in zip(dbl, has_b) if hb])


def fuse_weights(wl: Sequence[torch.Tensor], wr: Sequence[Optional[torch.Tensor]],
                 bl: Sequence[Optional[torch.Tensor]], scales: Sequence[float]
                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Differentiable fused weight of a destination update (see ``hgnn_fuse_weights``)."""
    ks = tuple(int(t.shape[1]) for t in wl)
    roots = [t for t in wr if t is not None]
    k_root = int(roots[0].shape[1]) if roots else 0
    meta = (ks, k_root, tuple(float(x) for x in scales), tuple(t is not None for t in wr),
            tuple(t is not None for t in bl))
    out = _FuseWeights.apply(meta, *wl, *roots, *[t for t in bl if t is not None])
    return out if isinstance(out, tuple) else (out, None)


class _FuseWeightsMulti(torch.autograd.Function):
    """``_FuseWeights`` for every destination update of a layer in one launch each way
    (``hgnn_fuse_weights_multi`` / ``hgnn_split_weight_grads_multi``): a layer's updates cost
    one fuse and one split launch instead of one each per update."""

    @staticmethod
    def forward(ctx, metas, *ts):
        h, dev = int(ts[0].shape[0]), ts[0].device
        outs, w_out, b_out, groups, i = [], [], [], [], 0
        for meta in metas:
            ks, k_root, scales, has_r, has_b = meta
            R = len(ks)
            n = R + sum(has_r) + sum(has_b)
            g = ts[i:i + n]
            i += n
            wl, it = list(g[:R]), iter(g[R:])
            wr = [next(it) if hr else None for hr in has_r]
            bl = [next(it) if hb else None for hb in has_b]
            groups.append((wl, wr, bl))
            W = torch.empty(h, sum(ks) + k_root, dtype=torch.float32, device=dev)
            b = torch.empty(h, dtype=torch.float32, device=dev) if any(has_b) else None
            w_out.append(W)
            b_out.append(b)
            outs.append(W)
            if b is not None:
                outs.append(b)
        plan = _fuse_multi_plan(metas, groups)
        N.check(N.lib().hgnn_fuse_weights_multi(
            len(metas), plan.a_nrel, plan.a_wl, plan.a_ks, plan.a_wr, plan.a_kroot, plan.a_bl,
            plan.a_sc, h, N.ptr_array(w_out), N.ptr_array(b_out), N.stream_ptr(dev)),
            "hgnn_fuse_weights_multi")
        ctx.metas, ctx.h, ctx.dev, ctx.plan = metas, h, dev, plan
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        need = ctx.needs_input_grad[1:]
        dws, dbs, dwl, dwr, dbl, ret = [], [], [], [], [], []
        gi = ni = 0
        for meta in ctx.metas:
            ks, k_root, scales, has_r, has_b = meta
            dW = grads[gi]
            gi += 1
            db = None
            if any(has_b):
                db = grads[gi]
                gi += 1
            if dW is None:
                dW = torch.zeros(ctx.h, sum(ks) + k_root, dtype=torch.float32, device=ctx.dev)
            if db is None and any(has_b):
                db = torch.zeros(ctx.h, dtype=torch.float32, device=ctx.dev)
            dws.append(dW.contiguous())
            dbs.append(None if db is None else db.contiguous())
            new = lambda shape, j: (torch.empty(shape, dtype=torch.float32, device=ctx.dev)
                                    if need[j] else None)
            gl = [new((ctx.h, k), ni + r) for r, k in enumerate(ks)]
            j = ni + len(ks)
            gr, gb = [], []
            for hr in has_r:
                gr.append(new((ctx.h, k_root), j) if hr else None)
                j += hr
            for hb in has_b:
                gb.append(new((ctx.h,), j) if hb else None)
                j += hb
            ni = j
            dwl += gl
            dwr += gr
            dbl += gb
            ret += gl + [t for t, hr in zip(gr, has_r) if hr] + [t for t, hb in zip(gb, has_b)
                                                                if hb]
        p = ctx.plan
        N.check(N.lib().hgnn_split_weight_grads_multi(
            len(ctx.metas), p.a_nrel, N.ptr_array(dws), N.ptr_array(dbs), p.a_ks, p.a_kroot,
            p.a_sc, ctx.h, N.ptr_array(dwl), N.ptr_array(dwr), N.ptr_array(dbl),
            N.stream_ptr(ctx.dev)), "hgnn_split_weight_grads_multi")
        return (None, *ret)


class _FuseMultiPlan:
    """The host arrays of one multi-update fuse (built once per set of parameter buffers)."""
    __slots__ = ("a_nrel", "a_wl", "a_wr", "a_bl", "a_ks", "a_sc", "a_kroot")

    def __init__(self, metas, groups):
        wl = [t for g in groups for t in g[0]]
        wr = [t for g in groups for t in g[1]]
        bl = [t for g in groups for t in g[2]]
        self.a_nrel = N.int_array([len(m[0]) for m in metas])
        self.a_wl, self.a_wr, self.a_bl = N.ptr_array(wl), N.ptr_array(wr), N.ptr_array(bl)
        self.a_ks = N.int_array([k for m in metas for k in m[0]])
        self.a_sc = N.float_array([x for m in metas for x in m[2]])
        self.a_kroot = N.int_array([m[1] for m in metas])


_FUSE_MULTI_PLANS: Dict[tuple, _FuseMultiPlan] = {}


def _fuse_multi_plan(metas, groups) -> _FuseMultiPlan:
    key = (metas, tuple(0 if t is None else t.data_ptr()
                        for g in groups for part in g for t in part))
    plan = _FUSE_MULTI_PLANS.get(key)
    if plan is None:
        if len(_FUSE_MULTI_PLANS) >= 1024:
            _FUSE_MULTI_PLANS.clear()
        plan = _FUSE_MULTI_PLANS[key] = _FuseMultiPlan(metas, groups)
    return plan


def fuse_weights_multi(groups) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """``fuse_weights`` for several destination updates (``groups``: (wl, wr, bl, scales) each,
    one hidden width) in one launch each way; one update, or more than 4, falls back to the
    per-update calls."""
    if len(groups) == 1 or len(groups) > 4:
        return [fuse_weights(*g) for g in groups]
    metas, flat = [], []
    for wl, wr, bl, scales in groups:
        ks = tuple(int(t.shape[1]) for t in wl)
        roots = [t for t in wr if t is not None]
        metas.append((ks, int(roots[0].shape[1]) if roots else 0,
                      tuple(float(x) for x in scales), tuple(t is not None for t in wr),
                      tuple(t is not None for t in bl)))
        flat += [*wl, *roots, *[t for t in bl if t is not None]]
    flat = [t.contiguous() for t in flat]     # (parameters are; the plan keys on addresses)
    outs = iter(_FuseWeightsMulti.apply(tuple(metas), *flat))
    return [(next(outs), next(outs) if any(m[4]) else None) for m in metas]


# ----------------------------------------------------------------------------- layer spec
@dataclasses.dataclass(frozen=True)
class DstGroup:
    dst: str
    rels: Tuple[Tuple[str, RelationCSR], ...]   # (source type, relation structure)
    root: bool                                   # x_dst segment present (root_weight)
    relu: bool
    # per relation: project the SOURCE table first (lin_l(mean x_j) == mean(lin_l x_j), bias
    # kept in the destination update) — see use_pre_projection
    pre: Tuple[bool, ...] = ()
    # destinations = the first n_root rows of the dst type's table (a sampled block: the next
    # layer's nodes lead the current ones); None: the whole table
    n_root: Optional[int] = None
    # the root segment is the whole input ``root_src`` instead (a block whose relations gather
    # from the global tables: its destinations' own rows come as a separate input)
    root_src: Optional[str] = None
    # per relation: the source table is a static model INPUT (first layer, no gradient, not
    # pre-projected), declared by the caller — its mean aggregate is kept across calls
    # (gather_mean's ``static``).  Never set for a deeper layer or a sampled block.
    static: Tuple[bool, ...] = ()


PRE_PROJECTION = os.environ.get("HGNN_PREPROJECT", "1") == "1"


def use_pre_projection(x_src: torch.Tensor, x_dst: torch.Tensor, hidden: int,
                       root: bool) -> bool:
    """Whether a relation's lin_l should run on its source table before the mean gather.

    The mean is linear, so ``W (mean_j x_j) = mean_j (W x_j)``: projecting the N_src source rows
    and gathering the projected rows replaces the [N_dst x d_src] part of the destination
    projection by an [N_src x d_src] one.  Worth it when the source table is at most half the
    destination table (cfg4 layer 2: 1M posts -> 9M users halves the user-side K3 flops, forward
    and backward) and the gathered rows do not widen (d_src >= hidden).  Only where the backward
    needs the source gradient anyway (``x_src.requires_grad``) or there is no backward: the
    projection's weight gradient is dP^T x_src with dP = the mean scatter's transpose of dz, a
    K2 pass the aggregate-first order does not need when x_src is a static input (layer 1).
    Rounding differs from the reference's order only at the fp32 ulp level.  HGNN_PREPROJECT=0
    turns it off."""
    if not (PRE_PROJECTION and root):
        return False
    if 2 * x_src.shape[0] > x_dst.shape[0] or x_src.shape[1] < hidden:
        return False
    return bool(x_src.requires_grad or not torch.is_grad_enabled())


@dataclasses.dataclass(frozen=True)
class LayerSpec:
    types: Tuple[str, ...]                       # order of node-feature inputs
    groups: Tuple[DstGroup, ...]
    # storage of the rows the layer's forward gathers: "fp32", "bf16", or None for ops.ROW_DTYPE
    # at call time (see ``_layer_plan``)
    row_dtype: Optional[str] = None
    # storage of the gradient rows the layer's K2 scatters read: "fp32", "bf16", or None for
    # ops.GRAD_ROW_DTYPE at call time (see ``_layer_plan``)
    grad_row_dtype: Optional[str] = None


# ----------------------------------------------------------------------------- layer plan
class _GroupPlan(NamedTuple):
    """What one destination group of a layer call does, every per-relation tuple normalised to
    one entry per relation."""
    dst: str
    rels: Tuple[Tuple[str, RelationCSR], ...]
    relu: bool
    root: bool                      # the destination rows' own features are a segment
    root_type: str                  # the input holding them
    prefix: Optional[int]           # they are its first ``prefix`` rows (a block); None: all
    n_dst: int                      # destination rows
    # relation i's lin_l runs on the source table and the projected rows are gathered
    pre: Tuple[bool, ...]
    # relation i's aggregate is kept across calls (never a pre-projected relation: that one
    # gathers the projected rows, which change with the weights)
    static: Tuple[bool, ...]
    bf16: Tuple[bool, ...]          # relation i gathers the bf16 copy of its table
    gbf16: Tuple[bool, ...]         # relation i's K2 reads the bf16 copy of its gradient table
    cols: Tuple[Tuple[int, int], ...]   # (offset, width) of relation i's lin_l block in the weight
    root_col: int                   # offset of the root block (the weight's last)
    main: Tuple[int, ...]           # the relations that are not pre-projected: the K3 segments


class _LayerPlan(NamedTuple):
    types: Tuple[str, ...]          # order of the node-feature inputs
    groups: Tuple[_GroupPlan, ...]
    # no group has a pre-projected relation: one K1 stage and one multi K3 call each way for the
    # layer.  Otherwise every group runs its own kernels one after the other.
    batched: bool
    shadow: Tuple[str, ...]         # source types gathered from a bf16 copy, in cast order


def _layer_plan(spec: LayerSpec, shapes: Dict[str, Tuple[int, int]], hidden: Sequence[int],
                bf16: bool, grad_bf16: bool = False) -> _LayerPlan:
    """Every decision of one ``hetero_layer`` call, from the spec, the inputs' ``(rows,
    columns)`` by type, each group's output width and the resolved row mode; no tensor is read.

    bf16 row mode: a relation gathers the bf16 copy of its table (the source table, or the
    projected rows of a pre-projected relation, so judged at the output width) only in a
    full-table group (a sampled block — ``n_root`` / ``root_src`` — keeps fp32 rows), never
    where the caller declared the table static (a model input is gathered once and kept,
    whatever HGNN_STATIC_AGG says), and only at a width that is a multiple of 8.

    bf16 gradient rows (``grad_bf16``): a relation's K2 reads the bf16 copy of its gradient
    table (dA at the segment width, or a pre-projected relation's dz at the output width) under
    the same two rules — a full-table group, a width that is a multiple of 8 — and where it has
    edges; whether its source needs a gradient (whether the K2 runs at all) is known only in the
    backward."""
    groups, shadow = [], []
    for gi, g in enumerate(spec.groups):
        block = g.n_root is not None or g.root_src is not None
        if any(g.static) and block:
            # a block's tables are buffers native kernels refill through raw pointers (no
            # version bump): an aggregate kept from them would be replayed stale
            raise ValueError("hetero_layer: a sampled block's relations are never static")
        R = range(len(g.rels))
        pre = tuple(bool(i < len(g.pre) and g.pre[i]) for i in R)
        if g.root_src is not None and (any(pre) or g.n_root is not None or not g.root):
            raise ValueError("hetero_layer: root_src takes a root segment, no n_root and no "
                             "pre-projected relation")
        root_type = g.dst if g.root_src is None else g.root_src
        n_dst = int(shapes[root_type][0] if g.n_root is None else g.n_root)
        for src, csr in g.rels:
            if csr.n_dst != n_dst or csr.n_src != shapes[src][0]:
                raise ValueError(f"hetero_layer: relation {src}->{g.dst} is {csr.n_src}->"
                                 f"{csr.n_dst} rows, the tables give {shapes[src][0]}->{n_dst}")
        static = tuple(bool(i < len(g.static) and g.static[i] and not pre[i]) for i in R)
        cols, o = [], 0
        for src, _ in g.rels:
            cols.append((o, int(shapes[src][1])))
            o += cols[-1][1]
        rounds = tuple(bool(bf16 and not block and not static[i]
                            and (hidden[gi] if pre[i] else cols[i][1]) % 8 == 0) for i in R)
        shadow += [g.rels[i][0] for i in R
                   if rounds[i] and not pre[i] and g.rels[i][0] not in shadow]
        grounds = tuple(bool(grad_bf16 and not block and g.rels[i][1].num_edges > 0
                             and (hidden[gi] if pre[i] else cols[i][1]) % 8 == 0) for i in R)
        groups.append(_GroupPlan(g.dst, tuple(g.rels), bool(g.relu), bool(g.root), root_type,
                                 g.n_root, n_dst, pre, static, rounds, grounds, tuple(cols), o,
                                 tuple(i for i in R if not pre[i])))
    return _LayerPlan(tuple(spec.types), tuple(groups), not any(any(p.pre) for p in groups),
                      tuple(shadow))


def _fresh_prefix(plan: _LayerPlan, gi: int, need_x: Dict[str, bool], k2_targets
                  ) -> Optional[int]:
    """Backward: group ``gi``'s root gradient goes into an unzeroed buffer of its input type —
    returns the number of rows the K3 dgrad writes (the block's roots) — or None: the buffer is
    zero-filled.  Fresh only in a batched layer, for a block given by ``n_root``, when K2s will
    add into that type (``k2_targets``): the first K2 round then adds into the prefix and writes
    the rows after it (``_k2_rounds``).  A block without roots is never fresh: the kernel's
    limit of 0 means "accumulate into every row", which would read the unwritten buffer."""
    p = plan.groups[gi]
    if not (plan.batched and p.root and p.prefix is not None and need_x[p.root_type]
            and p.root_type in k2_targets):
        return None
    return p.prefix if p.prefix > 0 else None


def _root(p: _GroupPlan, t: torch.Tensor) -> torch.Tensor:
    """The group's destination rows of ``t``, a tensor shaped like its root input (the features:
    the root segment; their gradient: what its dgrad writes): a prefix view in a block."""
    return t if p.prefix is None else t[:p.prefix]


def _main_weight(p: _GroupPlan, w: torch.Tensor) -> torch.Tensor:
    """The fused weight without the pre-projected relations' lin_l blocks."""
    if not any(p.pre):
        return w.contiguous()
    keep = [w[:, o:o + k] for o, k in (p.cols[i] for i in p.main)]
    if p.root:
        keep.append(w[:, p.root_col:])
    return torch.cat(keep, dim=1).contiguous()


def _fwd_job(p: _GroupPlan, xs, aggrs, w, b) -> FwdJob:
    """The K3 forward of a group over its main aggregates (+ root rows), with its mask buffer."""
    segs = list(aggrs) + ([_root(p, xs[p.root_type])] if p.root else [])
    mask = relu_mask_for(p.n_dst, int(w.shape[0]), p.relu, w.device,
                         sum(int(t.shape[1]) for t in segs))
    return FwdJob(segs, _main_weight(p, w), None if b is None else b.contiguous(), p.relu, mask)


def _main_dxs(p: _GroupPlan, aggrs, need_x, pending) -> List[Optional[torch.Tensor]]:
    """The gradient buffer of each main aggregate (None where no source gradient comes of it),
    each queued in ``pending`` for the K2 into its source type as ``(dA, csr, its K2 reads the
    bf16 copy of dA)``."""
    dxs: List[Optional[torch.Tensor]] = []
    for i, a in zip(p.main, aggrs):
        src, csr = p.rels[i]
        if need_x[src] and csr.num_edges > 0:
            dxs.append(torch.empty_like(a))
            pending.setdefault(src, []).append((dxs[-1], csr, p.gbf16[i]))
        else:
            dxs.append(None)
    return dxs


class _HeteroLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan: _LayerPlan, *flat):
        nt = len(plan.types)
        xs = dict(zip(plan.types, flat[:nt]))
        wb = flat[nt:]
        # bf16 row mode: one bf16 copy per distinct source table some relation of the layer
        # gathers, cast before any gather and held until the forward returns.  Nothing is saved
        # from them: the backward is the fp32 one, evaluated at the aggregates computed from the
        # rounded rows.
        shadow = {src: rows_to_bf16(xs[src]) for src in plan.shadow}

        def k1(p, i):
            src, csr = p.rels[i]
            if p.bf16[i]:
                return gather_mean(shadow[src], csr)
            return gather_mean(xs[src], csr, static=p.static[i], name=f"{src}->{p.dst}")

        def k1_group(p, w):
            """One group's gathers, relation by relation: its main aggregates, and the means of
            its pre-projected relations' P = x_src W_r^T summed into one [N_dst, h] input that
            the destination update adds in its epilogue."""
            aggrs, add = [], None
            for i, (src, csr) in enumerate(p.rels):
                if p.pre[i]:
                    o, k = p.cols[i]
                    P = linear_fwd([xs[src]], w[:, o:o + k].contiguous(), None, False)
                    if p.bf16[i]:
                        P = rows_to_bf16(P)    # rounded after the projection: the table the
                                               # gather reads
                    add = gather_mean(P, csr, out=add)
                    del P
                else:
                    aggrs.append(k1(p, i))
            return aggrs, add

        if plan.batched:
            if shadow:
                aggrs_by_g = [k1_group(p, None)[0] for p in plan.groups]
            else:
                # every relation's K1 of the layer in one launch (sampled blocks;
                # gather_mean_many falls back to one launch each where they do not qualify)
                many = iter(gather_mean_many(
                    [(xs[src], csr) for p in plan.groups for src, csr in p.rels],
                    static=[s for p in plan.groups for s in p.static],
                    names=[f"{src}->{p.dst}" for p in plan.groups for src, _ in p.rels]))
                aggrs_by_g = [[next(many) for _ in p.rels] for p in plan.groups]
            # and every destination type's K3 in one native call (the split path's column blocks
            # one launch for both types, hgnn_linear_fwd_multi)
            jobs = [_fwd_job(p, xs, aggrs, wb[2 * gi], wb[2 * gi + 1])
                    for gi, (p, aggrs) in enumerate(zip(plan.groups, aggrs_by_g))]
            outs = linear_fwd_many(jobs)
        else:
            aggrs_by_g, jobs, outs = [], [], []
            for gi, p in enumerate(plan.groups):
                aggrs, add = k1_group(p, wb[2 * gi])
                j = _fwd_job(p, xs, aggrs, wb[2 * gi], wb[2 * gi + 1])
                outs.append(linear_fwd(j.segs, j.w, j.b, j.relu, add=add, mask_out=j.mask))
                del add
                aggrs_by_g.append(aggrs)
                jobs.append(j)
        shadow.clear()
        ctx.plan = plan
        ctx.masks = [j.mask for j in jobs]   # ReLU bits of each output (None: no bit form)
        ctx.has_b = [b is not None for b in wb[1::2]]
        ctx.save_for_backward(*flat[:nt], *[t for t in wb if t is not None],
                              *[a for aggrs in aggrs_by_g for a in aggrs], *outs)
        return tuple(outs)

    @staticmethod
    def _saved(ctx):
        """``(xs, [(w, b)], main aggregates by group, outs)`` from what ``forward`` saved."""
        plan: _LayerPlan = ctx.plan
        saved = iter(ctx.saved_tensors)
        xs = {t: next(saved) for t in plan.types}
        wbs = [(next(saved), next(saved) if hb else None) for hb in ctx.has_b]
        aggrs_by_g = [[next(saved) for _ in p.main] for p in plan.groups]
        return xs, wbs, aggrs_by_g, list(saved)

    @staticmethod
    def backward(ctx, *douts):
        plan: _LayerPlan = ctx.plan
        nt, ng = len(plan.types), len(plan.groups)
        xs, wbs, aggrs_by_g, outs = _HeteroLayer._saved(ctx)
        need = ctx.needs_input_grad[1:]
        need_x = dict(zip(plan.types, need[:nt]))
        need_w = [need[nt + 2 * gi] for gi in range(ng)]
        need_b = [b is not None and need[nt + 2 * gi + 1] for gi, (_, b) in enumerate(wbs)]
        gx: Dict[str, Optional[torch.Tensor]] = {t: None for t in plan.types}
        gwb: List[Optional[torch.Tensor]] = [None] * (2 * ng)
        pending: Dict[str, list] = {}   # target type -> [(dA, csr)] for K2, after the roots
        # the types some K2 of this backward adds into: sources of the groups that got a
        # gradient.  (autograd materialises the gradient of an unused output as zeros, so through
        # ``hetero_layer`` every group has one today and a None ``dout`` is not reached)
        k2_targets = {src for p, dout in zip(plan.groups, douts) if dout is not None
                      for src, csr in p.rels if need_x[src] and csr.num_edges > 0}
        prefix: Dict[str, int] = {}     # type -> rows of its unzeroed gradient written so far
        # phase 1: every destination type's K3 backward; the groups with pre-projected
        # relations after the others (their root gradient adds into what those wrote)
        gis, jobs, pre_groups = [], [], []
        for gi, p in enumerate(plan.groups):
            if douts[gi] is None:
                continue
            if any(p.pre):
                pre_groups.append(gi)
                continue
            dxs = _main_dxs(p, aggrs_by_g[gi], need_x, pending)
            segs = list(aggrs_by_g[gi])
            if p.root:
                segs.append(_root(p, xs[p.root_type]))
                dxs.append(None)
                if need_x[p.root_type]:
                    fresh = _fresh_prefix(plan, gi, need_x, k2_targets)
                    if fresh is not None:
                        prefix[p.root_type] = fresh
                    dxs[-1] = _root_grad(p, xs, gx, fresh)
            gis.append(gi)
            jobs.append(BwdJob(segs, wbs[gi][0], douts[gi].contiguous(),
                               outs[gi] if p.relu else None, dxs, need_w[gi], need_b[gi],
                               ctx.masks[gi]))
        if plan.batched:
            # one native call for the destination types' K3 backward (hgnn_linear_bwd_multi)
            res = linear_bwd_many(jobs)
        else:
            res = [_linear_bwd_of(j) for j in jobs]
        for gi, (dw, db) in zip(gis, res):
            gwb[2 * gi], gwb[2 * gi + 1] = dw, db
        # groups with pre-projected relations: dz once, the destination update's backward on
        # it, then per pre-projected relation the K2 of dz into the projected source rows and
        # the projection's backward
        for gi in pre_groups:
            gwb[2 * gi], gwb[2 * gi + 1] = _pre_group_backward(
                plan.groups[gi], xs, aggrs_by_g[gi], wbs[gi][0], douts[gi].contiguous(), outs[gi],
                need_x, need_w[gi], need_b[gi], gx, pending, ctx.masks[gi])
        # phase 2: K2 per target type, as rounds of one launch each where they qualify
        for t in pending:
            if gx[t] is None:
                gx[t] = torch.zeros_like(xs[t])
        # (the rounds are sampled blocks' launches, fp32 rows: never with a bf16 gradient table)
        rounded = any(gb for items in pending.values() for _, _, gb in items)
        if rounded or not (len(pending) > 1 and _k2_rounds(
                {t: [(dA, csr) for dA, csr, _ in items] for t, items in pending.items()},
                gx, prefix)):
            for t, n in prefix.items():      # (no rounds after all: zero what K2s add into)
                gx[t][n:].zero_()
            if rounded:                      # (pending then holds the last reference to each dA)
                jobs.clear()
                dxs = None
            for t, items in pending.items():
                while items:
                    dA, csr, gb = items.pop(0)
                    if gb:
                        # bf16 gradient rows: cast just before the K2 that reads them, and the
                        # fp32 dA goes back to the allocator once the cast is enqueued
                        dA = rows_to_bf16(dA)
                    scatter_mean_bwd(dA, csr, out=gx[t])
                    del dA
        return (None, *[gx[t] for t in plan.types], *gwb)


def _root_grad(p: _GroupPlan, xs, gx, fresh: Optional[int] = None) -> torch.Tensor:
    """Allocates the gradient of the group's root input in ``gx`` and returns the rows the root
    segment's dgrad writes.  A block's rows after its roots are zero until the K2s add into
    them — or, with ``fresh`` (``_fresh_prefix``), left unwritten for the first K2 round."""
    zero = p.prefix is not None and fresh is None
    gx[p.root_type] = (torch.zeros_like if zero else torch.empty_like)(xs[p.root_type])
    return _root(p, gx[p.root_type])


def _k2_rounds(pending, gx, prefix=None) -> bool:
    """The K2s of a layer's backward as rounds of one launch each: round r takes the r-th
    relation of every target type (distinct outputs, so no two jobs of a launch add into the
    same rows; each target's relations keep their order).  ``prefix[t]``: gx[t] holds only its
    first rows (the root term); round 0 adds into those and writes the rest fresh.  False
    (nothing launched) where the relations do not qualify (source-blocked or heavy-row gathers,
    ``_multi_ok``)."""
    prefix = prefix or {}
    jobs_by_round: List[list] = []
    for t, items in pending.items():
        for r, (dA, csr) in enumerate(items):
            if csr.num_edges and gather_blocks(dA, csr.num_edges) > 1:
                return False
            if len(jobs_by_round) <= r:
                jobs_by_round.append([])
            jobs_by_round[r].append((dA.contiguous(), csr, gx[t]))
    for jobs in jobs_by_round:
        if len(jobs) > 1 and not _multi_ok([(dA, csr.bwd, o) for dA, csr, o in jobs]):
            return False
    if any(len(j) == 1 for j in jobs_by_round[:1]) and prefix:
        return False                         # round 0 must be a multi launch to honour prefix
    targets = list(pending)
    for r, jobs in enumerate(jobs_by_round):
        if len(jobs) == 1:
            dA, csr, o = jobs[0]
            scatter_mean_bwd(dA, csr, out=o)
        else:
            lim = None
            if r == 0 and prefix:
                lim = [prefix.get(t, 0) for t in targets if pending[t]]
            _gather_multi([(dA, csr.bwd, o) for dA, csr, o in jobs], mean=False,
                          accumulate=True, edge_ws=[csr.bwd_weights for _, csr, _ in jobs],
                          acc_limit=lim)
    return True


def relu_grad(dout: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """dz = dout * (out > 0): ReLU's backward from its output (one streaming pass)."""
    dz = torch.empty_like(dout)
    n = dout.numel()
    with _timed("relu_grad", 12 * n):
        N.check(N.lib().hgnn_hetero_epilogue_bwd(1, N.float_array([1.0]), n, 1, N.ptr(out),
                                                 N.ptr(dout), N.ptr_array([dz]),
                                                 N.stream_ptr(dout.device)),
                "hgnn_hetero_epilogue_bwd")
    return dz


def _pre_group_backward(g: _GroupPlan, xs, aggrs, w, dout, y, need_x, need_w, need_b, gx,
                        pending, mask=None):
    """Backward of a destination group with pre-projected relations: returns (dW, db) in the
    fused weight's column layout; source gradients go to ``gx`` / ``pending`` (K2 list)."""
    # the destination update's backward over the remaining segments also writes the masked dz
    # that the pre-projected relations' K2 scatters (from the pass that masks it anyway).  With
    # bf16 gradient rows those K2s read one bf16 dz cast straight from dout and the mask
    # (relu_grad_bf16), and K3 writes the fp32 dz only where some relation still reads it
    want16 = any(pre and gb for pre, gb in zip(g.pre, g.gbf16))
    want32 = any(pre and not gb for pre, gb in zip(g.pre, g.gbf16))
    dz = (torch.empty_like(dout) if want32 else None) if g.relu else dout
    segs = list(aggrs)
    seg_cols = [g.cols[i] for i in g.main]
    dxs = _main_dxs(g, aggrs, need_x, pending)
    dx_add = [False] * len(dxs)
    if g.root:
        segs.append(_root(g, xs[g.root_type]))
        seg_cols.append((g.root_col, int(w.shape[1]) - g.root_col))
        # the root gradient is added into the destination table's gradient in the dgrad pass
        # when another update already wrote it (no separate add); else it is that gradient
        # (a block's prefix of a zeroed table: its other rows wait for the K2s)
        held = need_x[g.root_type] and gx[g.root_type] is not None
        dx_add.append(held)
        if need_x[g.root_type]:
            dxs.append(_root(g, gx[g.root_type]) if held else _root_grad(g, xs, gx))
        else:
            dxs.append(None)
    dw = torch.empty_like(w) if need_w else None
    dw_main, db = linear_bwd(segs, _main_weight(g, w), dout, y if g.relu else None, dxs,
                             need_w, need_b, dz_out=dz if g.relu else None, mask=mask,
                             dx_add=dx_add)
    if dw is not None:
        o = 0
        for (co, k) in seg_cols:
            dw[:, co:co + k].copy_(dw_main[:, o:o + k])
            o += k
    # pre-projected relations: dP = K2(dz) over the CSC, then P = x_src W_r^T's backward
    dz16 = None
    if want16:       # once per group, however many relations read it
        if not g.relu:
            dz16 = rows_to_bf16(dout)
        elif mask is not None:
            dz16 = relu_grad_bf16(dout, mask=mask)
        else:
            dz16 = relu_grad_bf16(dout, out_act=y)
    for (src, csr), pre, gb, (o, k) in zip(g.rels, g.pre, g.gbf16, g.cols):
        if not pre:
            continue
        x_src = xs[src]
        dP = scatter_mean_bwd(dz16 if gb else dz, csr)
        add = need_x[src] and gx[src] is not None   # added into the table's gradient in place
        dxp = (gx[src] if add else torch.empty_like(x_src)) if need_x[src] else None
        dwp, _ = linear_bwd([x_src], w[:, o:o + k].contiguous(), dP, None, [dxp], need_w, False,
                            dx_add=[add])
        if dw is not None:
            dw[:, o:o + k].copy_(dwp)
        if dxp is not None:
            gx[src] = dxp
    return dw, db


def hetero_layer(spec: LayerSpec, x_dict: Dict[str, torch.Tensor],
                 weights: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]]
                 ) -> Dict[str, torch.Tensor]:
    plan = _layer_plan(spec, {t: tuple(x_dict[t].shape) for t in spec.types},
                       [int(w.shape[0]) for w, _ in weights],
                       resolve_row_dtype(spec.row_dtype) == "bf16",
                       resolve_grad_row_dtype(spec.grad_row_dtype) == "bf16")
    flat: List[Optional[torch.Tensor]] = [x_dict[t] for t in spec.types]
    for w, b in weights:
        flat.extend([w, b])
    N.require_device(*[t for t in flat if t is not None])
    for t in flat[:len(spec.types)]:
        _check_f32(t, "node features")
    outs = _HeteroLayer.apply(plan, *flat)
    return {p.dst: y for p, y in zip(plan.groups, outs)}


# ----------------------------------------------------------------------------- link loss
WEIGHTINGS = ("mean", "edge")


def _weighting_value(v: str, who: str) -> str:
    if v not in WEIGHTINGS:
        raise ValueError(f"{who}: weighting={v!r}; expected one of {WEIGHTINGS}")
    return v


def link_loss(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
              neg_p: torch.Tensor, pos_weights: torch.Tensor,
              weighting: str = "mean", logq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference training loss (train_gnn.py:259-281), on the device with torch ops.

    ``weighting="mean"``: ``BCEWithLogitsLoss()`` has mean reduction, so
    ``(pos_weights * pos_loss).mean()`` equals ``mean(pos_weights) * pos_loss`` — reproduced as
    written.  ``"edge"``: the positives' loss with ``reduction='none'``, so each positive edge's
    term (and gradient) carries its own weight,
    ``mean_e(w_e * softplus(-s_e)) + mean_e softplus(s_neg_e)``.

    ``neg_p`` of shape ``[E, k]``: k negatives per positive edge, the same lines with a 2-D draw;
    the negatives' term is then the mean over all E·k scores (``[E, 1]`` is ``[E]``).

    ``SkewedNegatives`` carry no order of their own here: pass their ``.values``, row e being the
    negatives of ``pos_edges[:, e]`` (for :func:`sample_negatives`' user-grouped draws, with the
    edges in that order).

    ``logq`` (floating ``[num_posts]``, e.g. :meth:`PostDistribution.log_q`): the logQ correction,
    every score less its post's entry (``pos_scores - logq[pos_p]``, ``neg_scores -
    logq[neg_p]``); a constant, no gradient flows into it.  Without it this is the function it
    was."""
    _weighting_value(weighting, "link_loss")
    if isinstance(neg_p, SkewedNegatives):
        raise TypeError("link_loss: pass SkewedNegatives.values, in the order of pos_edges")
    if logq is not None:
        _logq_rules(logq, int(post_emb.shape[0]), "link_loss")
    pos_u, pos_p = pos_edges[0], pos_edges[1]
    u = user_emb[pos_u]
    pos_scores = (u * post_emb[pos_p]).sum(dim=1)
    if neg_p.dim() == 2 and neg_p.shape[1] == 1:
        neg_p = neg_p.reshape(-1)
    if neg_p.dim() == 2:
        neg_scores = (u[:, None, :] * post_emb[neg_p]).sum(dim=-1)
    else:
        neg_scores = (u * post_emb[neg_p]).sum(dim=1)
    if logq is not None:
        b = logq.detach().to(pos_scores.dtype)
        pos_scores = pos_scores - b[pos_p]
        neg_scores = neg_scores - b[neg_p]
    crit = torch.nn.functional.binary_cross_entropy_with_logits
    neg_loss = crit(neg_scores, torch.zeros_like(neg_scores))
    if weighting == "edge":
        pos_loss = crit(pos_scores, torch.ones_like(pos_scores), reduction="none")
        return (pos_weights * pos_loss).mean() + neg_loss
    pos_loss = crit(pos_scores, torch.ones_like(pos_scores))
    return (pos_weights * pos_loss).mean() + neg_loss


# ----------------------------------------------------------------------------- fused link loss
def _user_of_pos(csr: RelationCSR) -> torch.Tensor:
    """Static per graph: the user owning each position of the user-grouped CSC (int32)."""
    m = getattr(csr, "_uop", None)
    if m is None:
        rp = csr.bwd.rowptr
        deg = (rp[1:] - rp[:-1]).long()
        m = torch.repeat_interleave(torch.arange(csr.n_src, dtype=torch.int32, device=rp.device),
                                    deg).contiguous()
        csr._uop = m
    return m


class EdgeWeights(NamedTuple):
    """The positives' per-edge weights (``weighting="edge"``) in the orders the two loss kernels
    walk: ``by_user[k]`` for position k of the user-grouped CSC (the scoring pass), ``by_post[p]``
    for position p of the post-grouped CSR (the dP gather); fp32, and ``one``: the device scalar
    1 that goes in as ``cscale``."""
    by_user: torch.Tensor
    by_post: torch.Tensor
    one: torch.Tensor


def edge_weights_in_kernel_order(csr: RelationCSR, pos_weights: torch.Tensor) -> EdgeWeights:
    """``pos_weights`` ([E], COO order) permuted once per graph, as ``_user_of_pos`` is built once:
    kept on the ``RelationCSR`` under the tensor's identity (held weakly and compared with ``is``:
    an id could be reused) and its ``_version``, so the same weights cost no per-step permutation
    and no host sync, and an in-place change rebuilds them.  2 x 4 B per edge."""
    hit = getattr(csr, "_edge_w", None)
    if hit is not None and hit[0]() is pos_weights and hit[1] == pos_weights._version:
        return hit[2]
    dev = N.require_device(pos_weights)
    w = pos_weights.detach().to(torch.float32)

    def ordered(perm):   # (a relation built from_csr: the positions are the edge ids)
        return w.clone() if perm is None else w[perm.long()].contiguous()

    ew = EdgeWeights(ordered(csr.bwd.perm), ordered(csr.fwd.perm),
                     torch.ones((), dtype=torch.float32, device=dev))
    csr._edge_w = (weakref.ref(pos_weights), pos_weights._version, ew)
    return ew


def _edge_weighting(who: str, weighting: str, pos_weights, n_edges: int, clashes) -> bool:
    """The ``weighting`` argument of the two loss entry points checked (before anything touches
    the device): whether it is "edge".  ``clashes``: {argument name: value} of the arguments
    that "edge" does not combine with, each None when not given."""
    if _weighting_value(weighting, who) == "mean":
        return False
    given = [k for k, v in clashes.items() if v is not None]
    if given:
        raise ValueError(f"{who}: weighting='edge' does not combine with {' / '.join(given)} "
                         "(the sharded step keeps the scalar cscale; the per-edge loss takes "
                         "its weights from pos_weights and its edge count from pos_edges)")
    if pos_weights is None or tuple(pos_weights.shape) != (n_edges,):
        raise ValueError(f"{who}: weighting='edge' needs pos_weights of shape [{n_edges}], one "
                         "per positive edge in COO order")
    return True


def _logq_rules(logq, n_posts: int, who: str, sharded=None) -> None:
    """The ``logq`` argument checked before anything touches the device: a floating tensor of
    shape ``[n_posts]``.  ``sharded``: {argument name: value} of the sharded step's arguments,
    which it does not combine with (each None when not given)."""
    if not isinstance(logq, torch.Tensor) or not logq.is_floating_point():
        raise ValueError(f"{who}: logq must be a floating tensor of shape [{n_posts}] "
                         f"(got {getattr(logq, 'dtype', type(logq).__name__)})")
    if tuple(logq.shape) != (n_posts,):
        raise ValueError(f"{who}: logq of shape {list(logq.shape)}; expected [{n_posts}], one "
                         "entry per post")
    given = [a for a, v in (sharded or {}).items() if v is not None]
    if given:
        raise ValueError(f"{who}: logq does not combine with {' / '.join(given)} (the sharded "
                         "step stays on the uncorrected scores)")


def logq_table(csr: RelationCSR, logq: torch.Tensor) -> torch.Tensor:
    """``logq`` as the table the two loss kernels read: detached, contiguous fp32, and checked
    finite — once per tensor object and ``_version``, kept on the ``RelationCSR`` the way
    :func:`edge_weights_in_kernel_order` keeps the weights (held weakly, compared with ``is``).
    The finite check is the one host sync, paid when the table is first seen or has changed in
    place, never per step."""
    hit = getattr(csr, "_logq", None)
    if hit is not None and hit[0]() is logq and hit[1] == logq._version:
        return hit[2]
    N.require_device(logq)
    t = logq.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("edge_bce_loss: logq must be finite (a post of weight 0 has no log; "
                         "PostDistribution.log_q gives it the smallest drawable weight's)")
    csr._logq = (weakref.ref(logq), logq._version, t)
    return t


def negatives_in_user_order(csr: RelationCSR, neg_p: torch.Tensor) -> torch.Tensor:
    """Re-order negatives drawn per COO edge (train_gnn.py:272) to the user-grouped order the
    fused kernel walks."""
    return neg_p.to(torch.int64)[csr.bwd.perm.long()].contiguous()


def _row_range(grouped, lo: int, hi: int):
    """Rows [lo, hi) of a grouping as a grouping of their own (rowptr slice with absolute offsets
    into the shared col), with its own skew plan — built once and cached on the grouping."""
    from .graph import GroupedEdges, _plan
    cache = grouped.__dict__.setdefault("_ranges", {})
    g = cache.get((lo, hi))
    if g is None:
        rp = grouped.rowptr[lo:hi + 1]
        g = cache[(lo, hi)] = GroupedEdges(rp, grouped.col, None, _plan(rp, hi - lo,
                                                                         grouped.plan.chunk),
                                           hi - lo)
    return g


class _Negatives(NamedTuple):
    """The loss's negatives in the user-grouped order, in exactly one of the three forms they
    come in: an int64 tensor (``torch.randint``'s), an int32 tensor (``sample_negatives``': in
    range by construction) or a ``NegativeDraw`` (drawn again wherever they are read: the sort's
    first pass, the scoring pass)."""
    i64: Optional[torch.Tensor]
    i32: Optional[torch.Tensor]
    draw: Optional["NegativeDraw"]
    k: int = 1      # negatives per positive edge: the tensors are row-major [E, k]
    planned: bool = False   # ``SkewedNegatives``: the dP gather plans their lists per step

    @classmethod
    def of(cls, neg_u_order, E: int, n_posts: int) -> "_Negatives":
        """``neg_u_order`` checked against the ``E`` positive edges and ``n_posts``."""
        k = _neg_count(neg_u_order, E, "edge_bce_loss")
        if isinstance(neg_u_order, SkewedNegatives):
            return cls(None, neg_u_order.values.contiguous(), None, k, True)
        if isinstance(neg_u_order, NegativeDraw):
            if neg_u_order.num_posts != n_posts:
                raise ValueError("edge_bce_loss: the NegativeDraw does not match the positive "
                                 "edges")
            return cls(None, None, neg_u_order, k)
        if neg_u_order.dtype == torch.int32:
            return cls(None, neg_u_order.contiguous(), None, k)
        return cls(neg_u_order.to(torch.int64).contiguous(), None, None, k)


def _neg_count(neg_p, E: int, who: str, sharded=None) -> int:
    """k of negatives given as ``[E]`` / ``[E, k]`` (a tensor or a ``NegativeDraw``), checked
    against the ``E`` positive edges before anything touches the device.  ``sharded``: {argument
    name: value} of the sharded step's callbacks, which k >= 2 does not combine with."""
    if isinstance(neg_p, NegativeDraw):
        k = neg_p.num_neg
        if neg_p.n != E * k:
            raise ValueError(f"{who}: the NegativeDraw does not match the positive edges (it "
                             f"draws {neg_p.n} = [{neg_p.n // k}, {k}] negatives; expected "
                             f"[{E}, {k}] for {E} positive edges)")
    else:
        shape = tuple(neg_p.shape)
        k = shape[1] if len(shape) == 2 else 1
        if len(shape) not in (1, 2) or shape[0] != E or k < 1:
            raise ValueError(f"{who}: neg_p of shape {list(shape)}; expected [{E}] (one negative "
                             f"per positive edge) or [{E}, k] (k per positive edge)")
    if E * k >= 2**31 - 1:
        raise ValueError(f"{who}: {E} positive edges x {k} negatives reach the negatives sort's "
                         "limit of 2^31 - 1 pairs")
    given = [a for a, v in (sharded or {}).items() if v is not None]
    if k >= 2 and given:
        raise ValueError(f"{who}: {k} negatives per positive edge do not combine with "
                         f"{' / '.join(given)} (the sharded step draws one negative per edge)")
    return k


def _user_of_draw(csr: RelationCSR, k: int) -> torch.Tensor:
    """The sort's payload: the user of each of the E·k negatives (row-major [E, k], user-grouped
    order).  k = 1 is ``_user_of_pos``; another k is built once per (graph, k) and kept on the
    ``RelationCSR`` beside it, 4·E·k bytes."""
    if k == 1:
        return _user_of_pos(csr)
    cache = csr.__dict__.setdefault("_uop_k", {})
    m = cache.get(k)
    if m is None:
        m = cache[k] = _user_of_pos(csr).repeat_interleave(k).contiguous()
    return m


def _sort_negatives(negs: _Negatives, uop, E: int, np_: int, err, dev):
    """The negatives (user-grouped order) grouped by post: (rowptr over posts, users in that
    order), stable — the order the dP gather sums them in.  ``E``: the number of (post, user)
    pairs, the positive edges times ``negs.k``; ``uop``: the user of each."""
    lib = N.lib()
    rowptr_n = torch.empty(np_ + 1, dtype=torch.int32, device=dev)
    nu_s = torch.empty(E, dtype=torch.int32, device=dev)
    ws = N.workspace(lib.hgnn_sort_pairs_ws_bytes(E, np_), dev)
    if negs.draw is not None:
        # draws computed in the sort's first pass (and again in the scoring pass: no
        # position-order copy is written)
        with _timed("sort_negatives", 4 * E * (2 * 4)):
            N.check(lib.hgnn_draw_sort_negatives(
                N.ptr(negs.draw.seed), N.ptr(uop), E, np_, None, N.ptr(rowptr_n),
                N.ptr(nu_s), N.ptr(ws), ws.numel(), N.stream_ptr(dev)),
                "hgnn_draw_sort_negatives")
    elif negs.i32 is not None:
        # int32 keys: no validation pass (the scoring pass below counts out-of-range
        # negatives; the sort only misplaces such a key, never dereferences it)
        with _timed("sort_negatives", 4 * E * (2 * 4) + 4 * E):
            N.check(lib.hgnn_sort_pairs_i32(
                N.ptr(negs.i32), N.ptr(uop), None, E, np_, N.ptr(rowptr_n), N.ptr(nu_s),
                None, None, N.ptr(ws), ws.numel(), N.stream_ptr(dev)),
                "hgnn_sort_pairs_i32")
    else:
        with _timed("sort_negatives", 4 * E * (2 + 1 + 4) + 4 * E):
            N.check(lib.hgnn_sort_pairs_i64(
                N.ptr(negs.i64), N.ptr(uop), None, E, np_, N.ptr(rowptr_n), N.ptr(nu_s),
                None, N.ptr(err[1:]), N.ptr(ws), ws.numel(), N.stream_ptr(dev)),
                "hgnn_sort_pairs_i64")
    return rowptr_n, nu_s


class PresortedNegatives:
    """The loss's negatives already grouped by post (``presort_negatives``): the sharded step
    sorts them under a collective, ahead of the loss that consumes them.  It holds the grouping
    and the draws it was made from (the objects themselves, compared with ``is``: an id could be
    reused by a new object once the old one is freed), so a loss over other edges or other
    draws is refused.  ``plan``: the ``_NegPlan`` of ``SkewedNegatives`` (made with the grouping,
    on the device), None for plain negatives; a loss over the other kind is refused."""

    def __init__(self, csr, neg_p, neg_order: str, n_posts: int, rowptr, users, k: int = 1,
                 plan=None):
        self.csr, self.neg_p, self.neg_order = csr, neg_p, neg_order
        self.n_posts = int(n_posts)
        self.rowptr, self.users = rowptr, users
        self.k = int(k)            # negatives per positive edge the grouping holds
        self.plan = plan

    @property
    def planned(self) -> bool:
        return self.plan is not None

    def check_draws(self, neg_p, neg_order: str, where: str) -> None:
        if isinstance(neg_p, SkewedNegatives) != self.planned:
            raise ValueError(f"{where}: the presorted negatives were grouped "
                             f"{'with' if self.planned else 'without'} a plan of their lists "
                             f"({'SkewedNegatives' if self.planned else 'plain negatives'}), the "
                             "loss got the other kind")
        if neg_order != self.neg_order:
            raise ValueError(f"{where}: presorted negatives were grouped with neg_order="
                             f"{self.neg_order!r}, the loss got neg_order={neg_order!r}")
        k = (neg_p.num_neg if isinstance(neg_p, NegativeDraw)
             else int(neg_p.shape[1]) if neg_p.dim() == 2 else 1)
        if k != self.k:
            raise ValueError(f"{where}: the presorted negatives hold {self.k} per positive edge, "
                             f"the loss got {k}")
        if neg_p is not self.neg_p:
            raise ValueError(f"{where}: presorted negatives of other draws")

    def check_edges(self, csr, n_posts: int, k: int = 1) -> None:
        if csr is not self.csr or int(n_posts) != self.n_posts:
            raise ValueError("edge_bce_loss: the presorted negatives are for other edges")
        if k != self.k:
            raise ValueError(f"edge_bce_loss: the presorted negatives hold {self.k} per positive "
                             f"edge, the loss got {k}")


def presort_negatives(n_users: int, n_posts: int, pos_edges: torch.Tensor, neg_p,
                      neg_order: str) -> PresortedNegatives:
    """The grouping ``edge_bce_loss_raw`` would sort its negatives into, done now (it needs
    only the edges and the draws, not the embeddings); pass it back as ``presorted=`` with the
    same ``neg_p`` and ``neg_order`` (required here: the two loss entry points default to
    different orders).  ``neg_p`` of shape ``[E, k]`` (or a ``NegativeDraw`` made for k): the
    grouping of all E·k negatives, for a loss over the same k.  ``SkewedNegatives``
    (``neg_order="user"``): the plan of their lists is made here too, on the device, and the
    loss must get the same ``SkewedNegatives``."""
    k = _neg_count(neg_p, int(pos_edges.shape[1]), "presort_negatives")
    csr = relation_csr_for_loss(pos_edges, n_users, n_posts)
    E = csr.num_edges
    negs = _Negatives.of(_negatives_user_order(csr, neg_p, neg_order), E, n_posts)
    dev = csr.fwd.rowptr.device
    err = torch.zeros(2, dtype=torch.int32, device=dev)
    rp, us = _sort_negatives(negs, _user_of_draw(csr, k), E * k, n_posts, err, dev)
    plan = _plan_negatives(rp, n_posts, E * k, csr.fwd.plan.chunk) if negs.planned else None
    return PresortedNegatives(csr, neg_p, neg_order, n_posts, rp, us, k, plan)


def _edge_bce(U, P, csr: RelationCSR, neg_u_order, cscale, check: bool, n_total: int,
              ready=None, on_dP=None, p_chunks=None, presorted=None, edge_w=None, logq=None):
    """Loss value and its gradients for a unit upstream gradient: (loss, dU, dP).  ``on_dP(dP)``,
    if given, is called once dP's kernels are enqueued and before the scoring pass (dU, the loss)
    is: the sharded step starts dP's reduce-scatter there, under the scoring pass.
    ``p_chunks`` (the sharded step): [(lo, hi, ready_fn)] — the post table arrives in row blocks
    (parallel.DistEnv.broadcast_slices_async); dP's rows [lo, hi) need only those rows of P, so
    the dP gather runs block by block as each lands (ready_fn: a stream wait), and the scoring
    pass, which reads all of P, after the last.

    ``U`` and ``P`` are fp32 tables, or both their bf16 copies (the bf16 row mode: both passes
    then read the bf16 rows, so the score <R(U[u]), R(P[p])> is one number in the scoring pass
    and in the dP gather; loss, dU and dP stay fp32).  The sharded step's arguments (``ready``,
    ``on_dP``, ``p_chunks``) are for fp32 rows only.

    ``edge_w``: ``EdgeWeights`` (``weighting="edge"``), the positives' per-edge weights in the two
    kernel orders; both passes then scale each positive edge by its own weight times ``cscale``.
    Not with the sharded step's arguments.

    ``neg_u_order`` of shape ``[E, k]`` (or a ``NegativeDraw`` made for k): k negatives per
    positive edge, row p those of user-grouped position p; ``n_total`` and ``cscale`` are given as
    for one negative and scaled here.  Not with the sharded step's arguments either.

    ``logq``: the table of :func:`logq_table` (fp32 ``[num_posts]``, or None): both passes then
    run their ``_lq`` entries, every logit its score less the post's entry.  Not with the sharded
    step's arguments."""
    sharded = ready is not None or on_dP is not None or p_chunks is not None
    if logq is not None and sharded:
        raise ValueError("edge_bce_loss: logq does not combine with ready / on_dP / p_chunks "
                         "(the sharded step stays on the uncorrected scores)")
    if edge_w is not None and sharded:
        raise ValueError("edge_bce_loss: weighting='edge' does not combine with ready / on_dP / "
                         "p_chunks (the sharded step keeps the scalar cscale)")
    U, P, relu_out = _loss_tables(U, P, csr, sharded)
    dev = N.require_device(U, P, neg_u_order, logq)
    np_, E = P.shape[0], csr.num_edges
    if E == 0:
        # a shard without positive edges (parallel.py): its share of the loss and gradients is
        # zero, and no kernel would read a negative (the C ABI rejects the empty tensor's null
        # pointer whenever the global edge count is non-zero)
        if ready is not None:
            ready()
        return (torch.zeros((), dtype=torch.float32, device=dev),
                torch.zeros(U.shape, dtype=torch.float32, device=dev),
                torch.zeros(P.shape, dtype=torch.float32, device=dev))
    negs = _Negatives.of(neg_u_order, E, np_)
    if negs.planned and sharded:
        raise ValueError("edge_bce_loss: SkewedNegatives do not combine with ready / on_dP / "
                         "p_chunks (the sharded step gathers dP by row blocks, without a plan)")
    if negs.k >= 2 and sharded:
        raise ValueError(f"edge_bce_loss: {negs.k} negatives per positive edge do not combine "
                         "with ready / on_dP / p_chunks (the sharded step draws one per edge)")
    # err[0]: zeroed and counted by the scoring pass, err[1] by the int64 negatives sort
    err = torch.empty(2, dtype=torch.int32, device=dev)
    c = cscale.to(torch.float32).reshape(()).contiguous()
    if negs.k >= 2:
        # The kernels weigh a positive edge c·inv_e and a negative inv_e.  With the edge count
        # n_total·k and the device scalar c·k (one tiny multiply, no host sync) those are c/E and
        # 1/(E·k): the mean over all E·k negatives, the positive term as with one negative.
        n_total, c = n_total * negs.k, c * float(negs.k)
    inv_e = 1.0 / n_total if n_total > 0 else 0.0
    dP = _loss_dP(U, P, csr, negs, c, inv_e, err, relu_out, ready, p_chunks, presorted,
                  edge_w.by_post if edge_w is not None else None, logq)
    if on_dP is not None:
        on_dP(dP)
    if ready is not None and p_chunks is not None:
        ready()                                 # all of P, for the scoring pass
    loss, dU = _loss_scoring_pass(U, P, csr, negs, c, n_total, err if check else None,
                                  edge_w.by_user if edge_w is not None else None, logq)
    if check and int(err[0]):
        raise ValueError("edge_bce_loss: negative post id out of range")
    return loss, dU, dP


def _loss_tables(U, P, csr: RelationCSR, sharded: bool):
    """``_edge_bce``'s tables checked: ``(U, P, whether U is marked a fused-ReLU output)``."""
    relu_out = bool(getattr(U, RELU_OUT, False))   # (read here: .contiguous() may copy)
    if U.dtype == torch.bfloat16:
        if P.dtype != torch.bfloat16:
            raise TypeError("edge_bce_loss: bf16 rows need both tables in bfloat16")
        if sharded:
            raise ValueError("edge_bce_loss: bf16 rows do not combine with ready / on_dP / "
                             "p_chunks (the sharded step runs on fp32 rows)")
        U, P = U.contiguous(), P.contiguous()
    else:
        U = _check_f32(U, "edge_bce_loss user_emb")
        P = _check_f32(P, "edge_bce_loss post_emb")
    if P.shape[1] != U.shape[1] or U.shape[0] != csr.n_src or P.shape[0] != csr.n_dst:
        raise ValueError("edge_bce_loss: embedding shapes do not match the positive edges")
    return U, P, relu_out


def _loss_dP(U, P, csr: RelationCSR, negs: _Negatives, c, inv_e, err, relu_out: bool, ready,
             p_chunks, presorted, edge_w=None, logq=None) -> torch.Tensor:
    """The dP chain: sort the negatives (post, user) by post, then both dP gathers in one pass,
    each edge's weight recomputed from <U[u], P[post]> (hgnn_score_gather2); the scoring pass
    (loss + dU) needs none of it.  ``ready`` / ``p_chunks``: see ``_edge_bce``.  ``edge_w``: the
    positives' weights in the post-grouped order (never with ``p_chunks``).  ``logq``: the fp32
    table, one offset per output row (never with ``ready`` / ``p_chunks``)."""
    from .graph import NO_SPLIT, GroupedEdges, Plan
    dev = U.device
    np_, E, pf = P.shape[0], csr.num_edges, csr.fwd
    dP = torch.empty(P.shape, dtype=torch.float32, device=dev)
    neg_plan = None
    if presorted is not None:
        presorted.check_edges(csr, np_, negs.k)
        if presorted.planned != negs.planned:
            raise ValueError("edge_bce_loss: the presorted negatives are of the other kind "
                             "(planned: SkewedNegatives; unplanned: plain negatives)")
        rowptr_n, nu_s, neg_plan = presorted.rowptr, presorted.users, presorted.plan
    else:
        rowptr_n, nu_s = _sort_negatives(negs, _user_of_draw(csr, negs.k), E * negs.k, np_, err,
                                         dev)
        if negs.planned:
            neg_plan = _plan_negatives(rowptr_n, np_, E * negs.k, pf.plan.chunk)
    if ready is not None and p_chunks is None:
        # P is still arriving (parallel.py's all-gather of the post table): the sort above
        # needs only the edges, so it ran ahead; every kernel below reads P
        ready()
    no_plan = Plan(NO_SPLIT, 0, 0, None, None)
    if p_chunks is not None:
        for lo, hi, rdy in p_chunks:
            if rdy is not None:
                rdy()
            if hi > lo:
                ng = GroupedEdges(rowptr_n[lo:hi + 1], nu_s, None, no_plan, hi - lo)
                _score_gather2(U, P[lo:hi], _row_range(pf, lo, hi), ng, c, inv_e, dP[lo:hi])
        return dP
    # (Measured and not kept, round 5: this gather in 8 source-block passes like K1,
    # 32.83 vs 31.32 ms at cfg4 — each pass re-reads its rows' P vectors and dP.)
    # A large post-ReLU U is more than half zeros: packed once (one streaming pass), the
    # gather's 2 E row reads fetch mask + non-zeros only (HGNN_ZPACK, csrc/zpack.h).
    Uz = None
    if U.dtype != torch.bfloat16 and ready is None and zpack_on(U, relu_out):
        Uz = zpack_rows(U)
    _score_gather2(U, P, pf, GroupedEdges(rowptr_n, nu_s, nu_s, no_plan, np_), c, inv_e, dP, Uz,
                   edge_w, neg_plan, logq)
    return dP


def _loss_scoring_pass(U, P, csr: RelationCSR, negs: _Negatives, c, n_total: int, err,
                       edge_w=None, logq=None):
    """``(loss, dU)``; ``err``: where it counts out-of-range negatives, or None; ``edge_w``: the
    positives' weights in the user-grouped order (the ``_w`` entries); ``logq``: the fp32 table
    (the ``_k_lq`` entries, for any k: the k kernel at k = 1 gives the one-negative results)."""
    # (The scoring pass takes no col_hot: with the positives' cold rows read nt it measured
    # 29-33 ms against 25.4 at cfg4 for every H tried)
    dev = U.device
    lib, s = N.lib(), N.stream_ptr(dev)
    nu, np_, d, E, ub = U.shape[0], P.shape[0], int(U.shape[1]), csr.num_edges, csr.bwd
    dU = torch.empty(U.shape, dtype=torch.float32, device=dev)
    part = torch.empty(int(lib.hgnn_edge_score_parts(nu)), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    head = (N.ptr(U), N.ptr(P), d, nu, np_, N.ptr(ub.rowptr), N.ptr(ub.col))
    tail = (N.ptr(part), N.ptr(loss), N.ptr(err), s)
    # per positive edge 1 + k post rows and 4 + 8k index bytes (k = 1: two rows, 12 B), per user
    # its own row in and a dU row out
    rb, k = _row_bytes(U), negs.k
    wb = 4 * E if edge_w is not None else 0
    wb += 4 * E * (1 + k) if logq is not None else 0      # one offset per scored pair
    with _timed(f"edge_score_d{d}", E * ((1 + k) * rb + 4 + 8 * k) + nu * (rb + 4 * d) + wb):
        if logq is not None:
            # (k = 1: n_total and c are unscaled, which is the convention at n_neg = 1)
            entry = ("hgnn_edge_score_fwd_k_lq_bf16" if U.dtype == torch.bfloat16
                     else "hgnn_edge_score_fwd_k_lq")
            N.check(getattr(lib, entry)(
                *head, N.ptr(edge_w), N.ptr(negs.i64), N.ptr(negs.i32),
                N.ptr(negs.draw.seed if negs.draw is not None else None), k, n_total, N.ptr(c),
                N.ptr(logq), N.ptr(dU), *tail), entry)
        elif k >= 2:
            # (n_total and c come scaled by k from _edge_bce: hgnn.h's convention)
            entry = ("hgnn_edge_score_fwd_k_bf16" if U.dtype == torch.bfloat16
                     else "hgnn_edge_score_fwd_k")
            N.check(getattr(lib, entry)(
                *head, N.ptr(edge_w), N.ptr(negs.i64), N.ptr(negs.i32),
                N.ptr(negs.draw.seed if negs.draw is not None else None), k, n_total, N.ptr(c),
                N.ptr(dU), *tail), entry)
        elif edge_w is not None:
            entry = ("hgnn_edge_score_fwd_w_bf16" if U.dtype == torch.bfloat16
                     else "hgnn_edge_score_fwd_w")
            N.check(getattr(lib, entry)(
                *head, N.ptr(edge_w), N.ptr(negs.i64), N.ptr(negs.i32),
                N.ptr(negs.draw.seed if negs.draw is not None else None), n_total, N.ptr(c),
                N.ptr(dU), *tail), entry)
        elif U.dtype == torch.bfloat16:
            N.check(lib.hgnn_edge_score_fwd_bf16(
                *head, N.ptr(negs.i64), N.ptr(negs.i32),
                N.ptr(negs.draw.seed if negs.draw is not None else None), n_total, N.ptr(c),
                N.ptr(dU), *tail), "hgnn_edge_score_fwd_bf16")
        elif negs.draw is not None:
            N.check(lib.hgnn_edge_score_fwd_draw(
                *head, N.ptr(negs.draw.seed), n_total, N.ptr(c), N.ptr(dU), *tail),
                "hgnn_edge_score_fwd_draw")
        elif negs.i32 is not None:
            N.check(lib.hgnn_edge_score_fwd_i32(
                *head, N.ptr(negs.i32), n_total, N.ptr(c), N.ptr(dU), *tail),
                "hgnn_edge_score_fwd_i32")
        else:
            N.check(lib.hgnn_edge_score_fwd(
                *head, N.ptr(negs.i64), None, n_total, N.ptr(c), N.ptr(dU), None, None, None,
                None, *tail), "hgnn_edge_score_fwd")
    return loss, dU


class _EdgeBCELoss(torch.autograd.Function):
    """The forward computes dL/dU and dL/dP with the loss (one scoring pass, one dP gather) and
    keeps them; the first backward scales them in place by the upstream gradient and hands them
    on (no copy: 2 x 4.6 GB at cfg4).  A second backward through a retained graph
    (``retain_graph=True``) recomputes them from the saved embeddings and the same negatives —
    the kernels are deterministic, so it returns what the first did, as torch's loss would.
    For that recompute U and P stay saved until the graph is freed (as torch's own loss saves
    its inputs): at cfg4 4.6 + 0.5 GB of the 288 GB, held from the forward to the end of the
    backward, which the split K3 backward (mask bits, not the outputs) would otherwise release
    after this loss's backward."""

    @staticmethod
    def forward(ctx, U, P, csr: RelationCSR, neg_u_order, cscale, check: bool, n_total: int,
                ready=None, presorted=None, bf16: bool = False, edge_w=None, logq=None):
        if bf16:
            # bf16 row mode: both passes read the bf16 copies, and those (half the bytes) are
            # what stays saved for the retained-graph recompute instead of U and P
            U, P = rows_to_bf16(U), rows_to_bf16(P)
        loss, dU, dP = _edge_bce(U, P, csr, neg_u_order, cscale, check, n_total, ready,
                                 presorted=presorted, edge_w=edge_w, logq=logq)
        ctx.grads = (dU, dP)
        ctx.save_for_backward(U, P)
        # (edge_w: the weights as this forward read them, in kernel order; a later in-place
        # change of the caller's tensor builds new ones and leaves these alone; logq: the fp32
        # table of logq_table, kept the same way)
        ctx.args = (csr, neg_u_order, cscale, n_total, edge_w, logq)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        if ctx.grads is None:        # retained graph, second backward: recompute
            U, P = ctx.saved_tensors
            csr, neg_u_order, cscale, n_total, edge_w, logq = ctx.args
            _, dU, dP = _edge_bce(U, P, csr, neg_u_order, cscale, False, n_total, edge_w=edge_w,
                                  logq=logq)
        else:
            dU, dP = ctx.grads
            ctx.grads = None         # handed on: autograd may accumulate into them from here
        if not getattr(go, UNIT_GRAD, False):
            g = go.to(torch.float32).reshape(()).contiguous()
            lib, s = N.lib(), N.stream_ptr(dU.device)
            for t in (dU, dP):   # in place; a no-op launch for loss.backward()'s gradient of 1
                N.check(lib.hgnn_scale_unless_one(N.ptr(t), t.numel(), N.ptr(g), s),
                        "hgnn_scale_unless_one")
        return dU, dP, None, None, None, None, None, None, None, None, None, None


# A tensor carrying this attribute (set True) is a gradient of exactly 1 that nobody writes:
# ``loss.backward(unit)`` with it skips the loss's scaling launches (minibatch.CapturedStep).
UNIT_GRAD = "_hgnn_unit_grad"


def unit_grad(device) -> torch.Tensor:
    """A scalar 1.0 marked ``UNIT_GRAD``, for ``loss.backward(unit)``: the fused loss then hands
    on its gradients unscaled, with no launch (the implicit ``loss.backward()`` makes a fill
    and, per gradient, a scale-by-1 launch — three graph nodes of a captured step)."""
    t = torch.ones((), dtype=torch.float32, device=device)
    setattr(t, UNIT_GRAD, True)
    return t


def edge_bce_loss(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
                  neg_p: torch.Tensor, pos_weights: Optional[torch.Tensor],
                  neg_order: str = "edge", check: bool = True,
                  n_edges_total: Optional[int] = None,
                  cscale: Optional[torch.Tensor] = None, ready=None,
                  presorted: Optional["PresortedNegatives"] = None,
                  row_dtype: Optional[str] = None, weighting: str = "mean",
                  logq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused HIP version of :func:`link_loss` (same value, same gradients).

    ``weighting``: "mean" (the default) is the reference's arithmetic, the weights collapsed to
    their mean; "edge" scales every positive edge's loss term and gradient by that edge's own
    ``pos_weights[e]`` (:func:`link_loss`'s ``weighting="edge"``), inside the same two kernels:
    ``pos_weights`` is then required with shape [E] in COO order, the kernels get ``cscale`` = 1,
    and ``cscale``, ``n_edges_total`` and ``ready`` (the sharded step's arguments) are errors.
    The weights are permuted to the kernels' orders once per graph and weights tensor
    (:func:`edge_weights_in_kernel_order`).  It combines with ``presorted``, every form of
    negatives, ``row_dtype="bf16"`` and ``HGNN_ZPACK``.

    ``neg_p`` of shape ``[E, k]`` (int64 or int32, or a ``NegativeDraw`` made with ``num_neg=k``):
    k negatives per positive edge, :func:`link_loss`'s 2-D form — the negatives' term is the mean
    over all E·k scores, the positive term is unchanged.  The scoring pass is then
    ``hgnn_edge_score_fwd_k`` (each positive row read once, U[u] kept in registers), the sort and
    the dP gather take the E·k (post, user) pairs.  ``[E]`` and ``[E, 1]`` are the one-negative
    path, bit for bit.  k >= 2 combines with both weightings, ``row_dtype="bf16"``,
    ``HGNN_ZPACK``, ``presorted``, ``check`` and ``n_edges_total`` / ``cscale``; with ``ready`` it
    is an error (the sharded step draws one negative per edge).

    ``neg_p`` a :class:`SkewedNegatives` (``neg_order="user"``; :func:`sample_negatives` with
    ``distribution`` / ``avoid``, or a caller's own int32 tensor marked that way): the same loss,
    the dP gather through ``hgnn_score_gather2_planned`` — the negatives' lists get a heavy-row
    plan on the device every step (no host sync), so draws piled on popular posts are summed by
    many waves.  It combines with both weightings, k >= 1, ``row_dtype="bf16"``, ``HGNN_ZPACK``
    and a ``presorted`` made from the same ``SkewedNegatives``; with ``ready`` it is an error.
    Plain tensors and ``NegativeDraw`` keep the unplanned gather.

    ``neg_order='edge'``: ``neg_p[e]`` is the negative of COO edge e (the reference's layout);
    ``'user'``: already in the user-grouped order (what :func:`sample_negatives` draws).
    ``check`` costs one host sync (the reference syncs every step with ``loss.item()``).
    ``n_edges_total`` / ``cscale`` (= mean of ALL pos_weights) let a shard of the positive edges
    produce its additive share of the global loss (parallel.py); ``ready()``, if given, is
    called once the negatives sort is enqueued and before any kernel reads ``post_emb`` (the
    sharded path's post-table all-gather finishes under the sort).  ``presorted``: the grouping
    of these negatives from :func:`presort_negatives`, done ahead (e.g. on a side stream under the
    forward; the caller orders the streams).

    ``row_dtype``: "fp32", "bf16" or None for ``ROW_DTYPE``.  With "bf16" both passes read bf16
    copies of the two tables (``_edge_bce``); the gradients pass straight through the rounding.
    A width that is no multiple of 8 keeps fp32 rows, and so does the sharded path (``ready``)
    under ``ROW_DTYPE`` — asking for "bf16" explicitly together with ``ready`` is an error.

    ``logq`` (floating ``[num_posts]`` on the tables' device, a constant: no gradient into it):
    the logQ correction of sampled losses.  Every scored pair, positive and negative alike, uses
    the logit ``<U[u], P[p]> - logq[p]`` in its loss term and its gradient coefficient, inside the
    same two kernels (``hgnn_edge_score_fwd_k_lq``, ``hgnn_score_gather2*_lq``): the scales, the
    sums, their order and determinism are unchanged.  :meth:`PostDistribution.log_q` gives
    ``log(k Q(p))`` for negatives drawn from it.  The tensor is detached, cast to contiguous fp32
    and checked finite once per tensor object and version (:func:`logq_table`; that check is the
    one host sync, not repeated per step); a wrong shape, a non-floating dtype or a non-finite
    entry is a ``ValueError``.  It combines with every form of negatives, k >= 1, both
    weightings, ``row_dtype="bf16"`` (the table stays fp32), ``HGNN_ZPACK``, ``presorted``
    (which does not depend on it), ``check`` and ``n_edges_total`` / ``cscale``; with ``ready``
    it is an error.  ``None`` runs exactly the code it ran before."""
    if logq is not None:
        _logq_rules(logq, int(post_emb.shape[0]), "edge_bce_loss", {"ready": ready})
    per_edge = _edge_weighting("edge_bce_loss", weighting, pos_weights, int(pos_edges.shape[1]),
                               {"cscale": cscale, "n_edges_total": n_edges_total,
                                "ready": ready})
    _neg_count(neg_p, int(pos_edges.shape[1]), "edge_bce_loss", {"ready": ready})
    _skewed_rules(neg_p, neg_order, "edge_bce_loss", {"ready": ready})
    bf16 = resolve_row_dtype(row_dtype) == "bf16"
    if bf16 and ready is not None:
        if row_dtype is not None:
            raise ValueError("edge_bce_loss: row_dtype='bf16' does not combine with ready (the "
                             "sharded step runs on fp32 rows)")
        bf16 = False
    bf16 = bf16 and user_emb.shape[1] % 8 == 0
    csr = relation_csr_for_loss(pos_edges, user_emb.shape[0], post_emb.shape[0])
    if neg_p.shape[0] != csr.num_edges:
        raise ValueError("one negative per positive edge is required (train_gnn.py:272)")
    neg_u = _negatives_user_order(csr, neg_p, neg_order)
    edge_w = edge_weights_in_kernel_order(csr, pos_weights) if per_edge else None
    if per_edge:
        cscale = edge_w.one
    elif cscale is None:
        cscale = pos_weights.to(torch.float32).mean()
    n_total = csr.num_edges if n_edges_total is None else int(n_edges_total)
    if presorted is not None:
        presorted.check_draws(neg_p, neg_order, "edge_bce_loss")
    if bf16:
        _check_f32(user_emb, "edge_bce_loss user_emb")
        _check_f32(post_emb, "edge_bce_loss post_emb")
    table = logq_table(csr, logq) if logq is not None else None
    return _EdgeBCELoss.apply(user_emb, post_emb, csr, neg_u, cscale, check, n_total, ready,
                              presorted, bf16, edge_w, table)


def edge_bce_loss_raw(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
                      neg_p: torch.Tensor, n_edges_total: Optional[int],
                      cscale: Optional[torch.Tensor],
                      neg_order: str = "user", ready=None, on_dP=None, p_chunks=None,
                      presorted: Optional[PresortedNegatives] = None, row_dtype: str = "fp32",
                      pos_weights: Optional[torch.Tensor] = None, weighting: str = "mean",
                      logq: Optional[torch.Tensor] = None):
    """:func:`edge_bce_loss` outside autograd: (loss, dL/dU, dL/dP) from the same kernels, for
    callers that run their own backward schedule (``parallel.UserShard.step``; ``on_dP``,
    ``p_chunks``: see ``_edge_bce``; ``presorted``: from :func:`presort_negatives` on the same
    edges and draws).  ``row_dtype`` is "fp32" unless asked otherwise (never ``ROW_DTYPE``:
    the sharded step stays on fp32 rows); "bf16" casts the two tables and runs both passes on the
    copies, and is an error together with ``p_chunks``, ``ready`` or ``on_dP``.

    ``weighting="edge"`` with ``pos_weights`` ([E], COO order): :func:`edge_bce_loss`'s per-edge
    mode and its rules — ``n_edges_total`` and ``cscale`` are then passed as None (the edge count
    is the positives', ``cscale`` is 1), and ``ready`` / ``on_dP`` / ``p_chunks`` are errors: the
    sharded step keeps the scalar ``cscale``.

    ``neg_p`` of shape ``[E, k]``: :func:`edge_bce_loss`'s k negatives per positive edge
    (``n_edges_total`` stays the number of positive edges); with k >= 2, ``ready`` / ``on_dP`` /
    ``p_chunks`` are errors.  A :class:`SkewedNegatives` (``neg_order="user"``): the planned dP
    gather, as in :func:`edge_bce_loss`; ``ready`` / ``on_dP`` / ``p_chunks`` are errors.

    ``logq``: :func:`edge_bce_loss`'s logQ table and its rules; with ``ready`` / ``on_dP`` /
    ``p_chunks`` it is an error, never a fallback to the uncorrected scores."""
    if logq is not None:
        _logq_rules(logq, int(post_emb.shape[0]), "edge_bce_loss_raw",
                    {"ready": ready, "on_dP": on_dP, "p_chunks": p_chunks})
    per_edge = _edge_weighting("edge_bce_loss_raw", weighting, pos_weights,
                               int(pos_edges.shape[1]),
                               {"cscale": cscale, "n_edges_total": n_edges_total, "ready": ready,
                                "on_dP": on_dP, "p_chunks": p_chunks})
    _neg_count(neg_p, int(pos_edges.shape[1]), "edge_bce_loss_raw",
               {"ready": ready, "on_dP": on_dP, "p_chunks": p_chunks})
    _skewed_rules(neg_p, neg_order, "edge_bce_loss_raw",
                  {"ready": ready, "on_dP": on_dP, "p_chunks": p_chunks})
    if not per_edge and (cscale is None or n_edges_total is None):
        raise ValueError("edge_bce_loss_raw: weighting='mean' needs n_edges_total and cscale")
    if _row_dtype_value(row_dtype, "row_dtype") == "bf16":
        if ready is not None or on_dP is not None or p_chunks is not None:
            raise ValueError("edge_bce_loss_raw: row_dtype='bf16' does not combine with "
                             "p_chunks / ready / on_dP (the sharded step runs on fp32 rows)")
        if user_emb.shape[1] % 8 == 0:
            user_emb = rows_to_bf16(_check_f32(user_emb, "edge_bce_loss_raw user_emb"))
            post_emb = rows_to_bf16(_check_f32(post_emb, "edge_bce_loss_raw post_emb"))
    csr = relation_csr_for_loss(pos_edges, user_emb.shape[0], post_emb.shape[0])
    neg_u = _negatives_user_order(csr, neg_p, neg_order)
    if presorted is not None:
        presorted.check_draws(neg_p, neg_order, "edge_bce_loss_raw")
    edge_w = None
    if per_edge:
        edge_w = edge_weights_in_kernel_order(csr, pos_weights)
        cscale, n_edges_total = edge_w.one, csr.num_edges
    table = logq_table(csr, logq) if logq is not None else None
    return _edge_bce(user_emb, post_emb, csr, neg_u, cscale, False, int(n_edges_total), ready,
                     on_dP, p_chunks, presorted, edge_w, table)


def _negatives_user_order(csr, neg_p, neg_order):
    if isinstance(neg_p, SkewedNegatives):
        if neg_order != "user":
            raise ValueError("SkewedNegatives are in the user-grouped order (neg_order='user')")
        return neg_p
    if isinstance(neg_p, NegativeDraw):
        if neg_order != "user":
            raise ValueError("a NegativeDraw is drawn in the user-grouped order (neg_order='user')")
        return neg_p
    return negatives_in_user_order(csr, neg_p) if neg_order == "edge" else neg_p.contiguous()


def relation_csr_for_loss(pos_edges, n_users, n_posts) -> RelationCSR:
    from .graph import relation_csr
    return relation_csr(pos_edges, n_users, n_posts)


# ------------------------------------------------------------------ sampled-softmax link loss
SOFTMAX_MAX_NEG = 63   # 1 + k logits of an edge fit a 64-column row of the kernel's LDS arrays


def _temperature_value(t, who: str) -> float:
    """``temperature`` checked before anything touches the device: a finite Python float > 0."""
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t <= 0:
        raise ValueError(f"{who}: temperature={t!r}; expected a finite Python float > 0 (a "
                         "learned temperature is not part of this loss)")
    return float(t)


def _softmax_neg_count(neg_p, E: int, who: str) -> int:
    k = _neg_count(neg_p, E, who)
    if k > SOFTMAX_MAX_NEG:
        raise ValueError(f"{who}: neg_p holds {k} negatives per positive edge; expected "
                         f"1 <= k <= {SOFTMAX_MAX_NEG}")
    return k


def link_softmax_loss(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
                      neg_p: torch.Tensor, pos_weights: Optional[torch.Tensor],
                      weighting: str = "mean", logq: Optional[torch.Tensor] = None,
                      temperature: float = 1.0) -> torch.Tensor:
    """The sampled-softmax (InfoNCE) link loss with torch ops: one (1 + k)-way classification
    per positive edge e = (u, p_0) against its negatives p_1 .. p_k (``neg_p`` of shape ``[E]`` or
    ``[E, k]``, row e those of ``pos_edges[:, e]``),

        z_j = <U[u], P[p_j]> / temperature - logq[p_j],    l_e = logsumexp_j(z_0 .. z_k) - z_0.

    ``weighting="mean"``: ``mean(pos_weights) * mean_e l_e``; ``"edge"``: ``mean_e(w_e * l_e)`` —
    the weight scales the whole edge term, there is no separate negatives' term.  ``logq``
    (floating ``[num_posts]``, e.g. :meth:`PostDistribution.log_q`): a constant, no gradient flows
    into it.  A negative id out of range takes no part in its edge's softmax; a negative equal to
    the edge's own positive is not masked.  :func:`edge_softmax_loss` is the fused HIP version."""
    _weighting_value(weighting, "link_softmax_loss")
    tau = _temperature_value(temperature, "link_softmax_loss")
    if isinstance(neg_p, SkewedNegatives):
        raise TypeError("link_softmax_loss: pass SkewedNegatives.values, in the order of pos_edges")
    _softmax_neg_count(neg_p, int(pos_edges.shape[1]), "link_softmax_loss")
    n_posts = int(post_emb.shape[0])
    if logq is not None:
        _logq_rules(logq, n_posts, "link_softmax_loss")
    pos_u, pos_p = pos_edges[0].long(), pos_edges[1].long()
    ids = torch.cat([pos_p[:, None], neg_p.reshape(pos_p.numel(), -1).long()], dim=1)
    valid = (ids >= 0) & (ids < n_posts)
    ids = torch.where(valid, ids, torch.zeros_like(ids))
    z = (user_emb[pos_u][:, None, :] * post_emb[ids]).sum(dim=-1) / tau
    if logq is not None:
        z = z - logq.detach().to(z.dtype)[ids]
    z = z.masked_fill(~valid, float("-inf"))
    term = torch.logsumexp(z, dim=1) - z[:, 0]
    if weighting == "edge":
        return (pos_weights * term).mean()
    c = 1.0 if pos_weights is None else pos_weights.to(term.dtype).mean()
    return c * term.mean()


def _softmax_slot_of(csr: RelationCSR) -> torch.Tensor:
    """Static per graph: the post-grouped position of each user-grouped position (int32 ``[E]``),
    where the scoring pass puts the positives' coefficients for the dP gather to read in its own
    order.  From the two groupings' ``perm`` (None: the identity, as in
    :func:`edge_weights_in_kernel_order`); kept on the ``RelationCSR``."""
    m = getattr(csr, "_slot_of", None)
    if m is None:
        fp, bp = csr.fwd.perm, csr.bwd.perm
        E, dev = csr.num_edges, csr.fwd.rowptr.device
        ident = torch.arange(E, dtype=torch.int32, device=dev)
        if fp is None:
            inv = ident
        else:
            inv = torch.empty(E, dtype=torch.int32, device=dev)
            inv[fp.long()] = ident
        m = (inv if bp is None else inv[bp.long()]).contiguous()
        csr._slot_of = m
    return m


def _edge_softmax(U, P, csr: RelationCSR, neg_u_order, cscale, check: bool, edge_w, logq,
                  tau: float):
    """Loss value and its gradients for a unit upstream gradient: ``(loss, dU, dP)``.

    Three steps, in this order (the BCE path's reverse order served the sharded step's overlap,
    which this path does not have): the scoring pass ``hgnn_edge_softmax_fwd`` (loss, dU and
    every pair's coefficient); the negatives' (post, user) pairs sorted by post with the
    coefficient's bits as the sort's second payload; ``hgnn_plan_device`` over the sorted lists
    and ``hgnn_coef_gather2_planned``, which reads each pair's weight instead of recomputing it.
    The lists are planned every step for every form of negatives.

    ``U`` / ``P``: fp32 tables or both their bf16 copies.  ``neg_u_order``: the negatives in the
    user-grouped order, ``[E]`` / ``[E, k]``.  A ``NegativeDraw`` is materialised once with the
    uniform-draw kernel (``hgnn_uniform_i32``) and sorted as int32: ``hgnn_draw_sort_negatives``
    has no second payload slot for the coefficient."""
    U, P, relu_out = _loss_tables(U, P, csr, False)
    dev = N.require_device(U, P, logq)
    lib, s = N.lib(), N.stream_ptr(dev)
    nu, np_, d, E = U.shape[0], P.shape[0], int(U.shape[1]), csr.num_edges
    if E == 0:
        return (torch.zeros((), dtype=torch.float32, device=dev),
                torch.zeros(U.shape, dtype=torch.float32, device=dev),
                torch.zeros(P.shape, dtype=torch.float32, device=dev))
    k = _softmax_neg_count(neg_u_order, E, "edge_softmax_loss")
    n = E * k
    i64 = i32 = None
    if isinstance(neg_u_order, NegativeDraw):
        if neg_u_order.num_posts != np_:
            raise ValueError("edge_softmax_loss: the NegativeDraw does not match the positive "
                             "edges")
        i32 = neg_u_order.tensor()
    elif isinstance(neg_u_order, SkewedNegatives):
        i32 = neg_u_order.values.contiguous()
    elif neg_u_order.dtype == torch.int32:
        i32 = neg_u_order.contiguous()
    else:
        i64 = neg_u_order.to(torch.int64).contiguous()
    N.require_device(U, i32, i64)
    # err[0]: zeroed and counted by the scoring pass, err[1] by the int64 negatives sort
    err = torch.empty(2, dtype=torch.int32, device=dev)
    c = cscale.to(torch.float32).reshape(()).contiguous()
    bf16 = U.dtype == torch.bfloat16
    ub, pf = csr.bwd, csr.fwd
    # ---- scoring pass: BCE's bytes, 4 B out per scored pair and the 4-B index of the positives'
    dU = torch.empty(U.shape, dtype=torch.float32, device=dev)
    coef_pos = torch.empty(E, dtype=torch.float32, device=dev)
    coef_neg = torch.empty(n, dtype=torch.float32, device=dev)
    part = torch.empty(int(lib.hgnn_softmax_parts(nu)), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    rb = _row_bytes(U)
    ib = 4 if i32 is not None else 8
    wb = (4 * E if edge_w is not None else 0) + (4 * E * (1 + k) if logq is not None else 0)
    with _timed(f"edge_softmax_d{d}", E * ((1 + k) * rb + 4 + ib * k) + nu * (rb + 4 * d) + wb
                + 4 * E * (1 + k) + 4 * E):
        N.check(lib.hgnn_edge_softmax_fwd(
            1 if bf16 else 0, N.ptr(U), N.ptr(P), d, nu, np_, N.ptr(ub.rowptr), N.ptr(ub.col),
            N.ptr(edge_w.by_user if edge_w is not None else None), N.ptr(i64), N.ptr(i32), k, E,
            N.ptr(c), N.ptr(logq), tau, N.ptr(_softmax_slot_of(csr)), N.ptr(dU), N.ptr(coef_pos),
            N.ptr(coef_neg), N.ptr(part), N.ptr(loss), N.ptr(err if check else None), s),
            "hgnn_edge_softmax_fwd")
    # ---- the negatives by post, users and coefficients (as int32 bits) in that order, stable
    rowptr_n = torch.empty(np_ + 1, dtype=torch.int32, device=dev)
    nu_s = torch.empty(n, dtype=torch.int32, device=dev)
    coef_s = torch.empty(n, dtype=torch.float32, device=dev)
    uop = _user_of_draw(csr, k)
    ws = N.workspace(lib.hgnn_sort_pairs_ws_bytes(n, np_), dev)
    if i32 is not None:
        # check=True: no validation pass over the keys (the scoring pass counted the ids out of
        # range, and the call raises on any).  check=False: such a key must leave the lists, so
        # the sort validates (one more pass over the keys) and drops it
        with _timed("sort_negatives_coef", 4 * n * (3 * 4) + 4 * n + (0 if check else 8 * n)):
            N.check(lib.hgnn_sort_pairs_i32(
                N.ptr(i32), N.ptr(uop), N.ptr(coef_neg), n, np_, N.ptr(rowptr_n), N.ptr(nu_s),
                N.ptr(coef_s), N.ptr(None if check else err[1:]), N.ptr(ws), ws.numel(), s),
                "hgnn_sort_pairs_i32")
    else:
        with _timed("sort_negatives_coef", 4 * n * (2 + 1 + 6) + 4 * n):
            N.check(lib.hgnn_sort_pairs_i64(
                N.ptr(i64), N.ptr(uop), N.ptr(coef_neg), n, np_, N.ptr(rowptr_n), N.ptr(nu_s),
                N.ptr(coef_s), N.ptr(err[1:]), N.ptr(ws), ws.numel(), s), "hgnn_sort_pairs_i64")
    plan = _plan_negatives(rowptr_n, np_, n, pf.plan.chunk)
    # ---- dP: E (1 + k) rows of U and 8 B (index, coefficient) per pair, no P rows
    Uz = zpack_rows(U) if not bf16 and zpack_on(U, relu_out) else None
    rows, table = (1, U) if bf16 else (2, Uz) if Uz is not None else (0, U)
    dP = torch.empty(P.shape, dtype=torch.float32, device=dev)
    neg_slab = torch.empty(max(2 * plan.max_heavy, 1) * d, dtype=torch.float32, device=dev)
    pairs = E + n
    nb = pairs * (rb + 8) + 8 * (np_ + 1) + 4 * np_ * d
    with _timed(f"coef_gather_planned[{np_}<-{nu}]x{d}", nb):
        N.check(lib.hgnn_coef_gather2_planned(
            rows, N.ptr(table), nu, d, N.ptr(pf.rowptr), N.ptr(pf.col), N.ptr(coef_pos),
            N.ptr(rowptr_n), N.ptr(nu_s), N.ptr(coef_s), np_, *_plan_args(pf.plan, d, dev),
            N.ptr(plan.heavy_rows), N.ptr(plan.heavy_first), N.ptr(plan.counts), plan.max_heavy,
            N.ptr(neg_slab), N.ptr(dP), s), "hgnn_coef_gather2_planned")
    if check and int(err[0]):
        raise ValueError("edge_softmax_loss: negative post id out of range")
    return loss, dU, dP


class _EdgeSoftmaxLoss(torch.autograd.Function):
    """``_EdgeBCELoss``'s scheme for the softmax loss: the forward computes dL/dU and dL/dP with
    the loss and keeps them; the first backward scales them in place by the upstream gradient
    and hands them on; a second backward through a retained graph recomputes them from the saved
    tables (the bf16 copies in the bf16 row mode) and the same negatives."""

    @staticmethod
    def forward(ctx, U, P, csr: RelationCSR, neg_u_order, cscale, check: bool, bf16: bool,
                edge_w, logq, tau: float):
        if bf16:
            U, P = rows_to_bf16(U), rows_to_bf16(P)
        loss, dU, dP = _edge_softmax(U, P, csr, neg_u_order, cscale, check, edge_w, logq, tau)
        ctx.grads = (dU, dP)
        ctx.save_for_backward(U, P)
        ctx.args = (csr, neg_u_order, cscale, edge_w, logq, tau)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        if ctx.grads is None:        # retained graph, second backward: recompute
            U, P = ctx.saved_tensors
            csr, neg_u_order, cscale, edge_w, logq, tau = ctx.args
            _, dU, dP = _edge_softmax(U, P, csr, neg_u_order, cscale, False, edge_w, logq, tau)
        else:
            dU, dP = ctx.grads
            ctx.grads = None         # handed on: autograd may accumulate into them from here
        if not getattr(go, UNIT_GRAD, False):
            g = go.to(torch.float32).reshape(()).contiguous()
            lib, s = N.lib(), N.stream_ptr(dU.device)
            for t in (dU, dP):   # in place; a no-op launch for loss.backward()'s gradient of 1
                N.check(lib.hgnn_scale_unless_one(N.ptr(t), t.numel(), N.ptr(g), s),
                        "hgnn_scale_unless_one")
        return dU, dP, None, None, None, None, None, None, None, None


def _softmax_args(who: str, user_emb, post_emb, pos_edges, neg_p, pos_weights, neg_order: str,
                  weighting: str, logq, temperature):
    """The argument rules of the two softmax entry points, all before anything touches the
    device: ``(csr, negatives in the user-grouped order, cscale, EdgeWeights or None, logq table
    or None, temperature)``."""
    tau = _temperature_value(temperature, who)
    E = int(pos_edges.shape[1])
    if logq is not None:
        _logq_rules(logq, int(post_emb.shape[0]), who)
    per_edge = _edge_weighting(who, weighting, pos_weights, E, {})
    _softmax_neg_count(neg_p, E, who)
    _skewed_rules(neg_p, neg_order, who, {})
    if neg_order not in ("edge", "user"):
        raise ValueError(f"{who}: neg_order={neg_order!r}; expected 'edge' or 'user'")
    csr = relation_csr_for_loss(pos_edges, user_emb.shape[0], post_emb.shape[0])
    neg_u = _negatives_user_order(csr, neg_p, neg_order)
    edge_w = edge_weights_in_kernel_order(csr, pos_weights) if per_edge else None
    if per_edge:
        cscale = edge_w.one
    elif pos_weights is None:
        cscale = torch.ones((), dtype=torch.float32, device=user_emb.device)
    else:
        cscale = pos_weights.to(torch.float32).mean()
    table = logq_table(csr, logq) if logq is not None else None
    return csr, neg_u, cscale, edge_w, table, tau


def edge_softmax_loss(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
                      neg_p, pos_weights: Optional[torch.Tensor], neg_order: str = "edge",
                      check: bool = True, row_dtype: Optional[str] = None,
                      weighting: str = "mean", logq: Optional[torch.Tensor] = None,
                      temperature: float = 1.0) -> torch.Tensor:
    """Fused HIP version of :func:`link_softmax_loss` (same value, same gradients): the sampled
    softmax over each positive edge and its k negatives, 1 <= k <= 63, with a temperature.

    ``neg_p`` comes in every form :func:`edge_bce_loss` takes — int64 / int32 ``[E]`` or
    ``[E, k]`` tensors, a ``NegativeDraw``, ``SkewedNegatives`` — with ``neg_order`` as there; the
    same ids give bitwise the same results in every form.  Mined hard negatives
    (:func:`mine_hard_negatives`) and popularity-weighted draws (:func:`sample_negatives` with
    ``distribution`` / ``avoid``) are the expected input, so the negatives' lists per post get a
    heavy-row plan on the device every step, whatever their form.  ``weighting``, ``logq`` and
    ``row_dtype`` are :func:`edge_bce_loss`'s (``logq=dist.log_q(k)`` is the correction this loss
    was invented with; with "edge" the weight scales the whole edge term); ``temperature`` is a
    finite Python float > 0, not a tensor.  ``check=True`` raises on a negative id out of range
    (one host sync); with ``check=False`` such a negative takes no part in its edge's softmax.
    Accidental hits (a negative equal to the edge's positive) are not masked.

    One scoring pass (``hgnn_edge_softmax_fwd``: every post row read once, an online softmax per
    edge, dU without atomics) emits each pair's gradient coefficient, the negatives' sort carries
    it as a payload, and ``hgnn_coef_gather2_planned`` sums dP from it (``_edge_softmax``).
    ``HGNN_ZPACK`` applies to the gather's user rows as in :func:`edge_bce_loss`.  The sharded
    step's arguments and ``presorted=`` are not part of this loss."""
    who = "edge_softmax_loss"
    bf16 = resolve_row_dtype(row_dtype) == "bf16" and user_emb.shape[1] % 8 == 0
    csr, neg_u, cscale, edge_w, table, tau = _softmax_args(
        who, user_emb, post_emb, pos_edges, neg_p, pos_weights, neg_order, weighting, logq,
        temperature)
    if bf16:
        _check_f32(user_emb, f"{who} user_emb")
        _check_f32(post_emb, f"{who} post_emb")
    return _EdgeSoftmaxLoss.apply(user_emb, post_emb, csr, neg_u, cscale, check, bf16, edge_w,
                                  table, tau)


def edge_softmax_loss_raw(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
                          neg_p, pos_weights: Optional[torch.Tensor], neg_order: str = "edge",
                          check: bool = True, row_dtype: str = "fp32", weighting: str = "mean",
                          logq: Optional[torch.Tensor] = None, temperature: float = 1.0):
    """:func:`edge_softmax_loss` outside autograd: ``(loss, dL/dU, dL/dP)`` from the same
    kernels.  ``row_dtype`` is "fp32" unless asked otherwise (never ``ROW_DTYPE``), as
    :func:`edge_bce_loss_raw`'s."""
    who = "edge_softmax_loss_raw"
    bf16 = _row_dtype_value(row_dtype, "row_dtype") == "bf16" and user_emb.shape[1] % 8 == 0
    csr, neg_u, cscale, edge_w, table, tau = _softmax_args(
        who, user_emb, post_emb, pos_edges, neg_p, pos_weights, neg_order, weighting, logq,
        temperature)
    if bf16:
        user_emb = rows_to_bf16(_check_f32(user_emb, f"{who} user_emb"))
        post_emb = rows_to_bf16(_check_f32(post_emb, f"{who} post_emb"))
    return _edge_softmax(user_emb, post_emb, csr, neg_u, cscale, check, edge_w, table, tau)


class NegativeDraw:
    """Uniform negative posts per positive edge (one, or ``num_neg``: row-major [E, num_neg], draw
    p·num_neg + j being negative j of user-grouped position p), not yet materialised: the device
    seed of a counter-based draw (:func:`draw_negatives`).  The fused loss draws and groups them by
    post in one call (``hgnn_draw_sort_negatives``: the draws are computed inside the sort's first
    pass, not written by one kernel and read back by two); :meth:`tensor` gives the same int32
    values as :func:`sample_negatives` would for the same seed.  ``n``: the number of draws."""

    def __init__(self, seed: torch.Tensor, n: int, num_posts: int, num_neg: int = 1):
        self.seed, self.n, self.num_posts = seed, int(n), int(num_posts)
        self.num_neg = _num_neg_value(num_neg)
        if self.n % self.num_neg:
            raise ValueError(f"NegativeDraw: {self.n} draws are no multiple of num_neg={num_neg}")
        self.shape = (self.n,) if self.num_neg == 1 else (self.n // self.num_neg, self.num_neg)
        self.dtype = torch.int32
        self.device = seed.device

    def tensor(self) -> torch.Tensor:
        out = torch.empty(self.shape, dtype=torch.int32, device=self.device)
        if self.n:
            N.check(N.lib().hgnn_uniform_i32(N.ptr(self.seed), self.n, self.num_posts, N.ptr(out),
                                             N.stream_ptr(self.device)), "hgnn_uniform_i32")
        return out


class SkewedNegatives:
    """Negatives whose lists per post may be far from even (drawn by popularity,
    :func:`sample_negatives` with ``distribution`` / ``avoid``): a thin holder of the int32
    ``[E]`` / ``[E, k]`` tensor in the user-grouped order (``.values``).  The loss entry points
    take it with ``neg_order="user"`` and give the dP gather a per-step plan of the negatives'
    lists, so a post drawn a million times is summed by many waves and not by one.
    ``SkewedNegatives(tensor)`` marks negatives of the caller's own that way; the plain-torch
    :func:`link_loss` takes ``.values`` in the order of its edges."""

    def __init__(self, values: torch.Tensor):
        if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or \
                values.dim() not in (1, 2):
            raise ValueError("SkewedNegatives: an int32 tensor of shape [E] or [E, k] in the "
                             "user-grouped order is required")
        self.values = values

    @property
    def shape(self):
        return self.values.shape

    @property
    def dtype(self):
        return self.values.dtype

    @property
    def device(self):
        return self.values.device

    def dim(self) -> int:
        return self.values.dim()


def _skewed_rules(neg_p, neg_order: str, who: str, sharded) -> None:
    """``SkewedNegatives`` checked before anything touches the device: the user-grouped order
    only, and never with the sharded step's arguments ({name: value}, None when not given)."""
    if not isinstance(neg_p, SkewedNegatives):
        return
    if neg_order != "user":
        raise ValueError(f"{who}: SkewedNegatives are in the user-grouped order "
                         "(neg_order='user')")
    given = [a for a, v in sharded.items() if v is not None]
    if given:
        raise ValueError(f"{who}: SkewedNegatives do not combine with {' / '.join(given)} (the "
                         "sharded step gathers dP by row blocks, without a plan of the "
                         "negatives' lists)")


class PostDistribution:
    """A distribution over the posts to draw negatives from (:func:`sample_negatives`), as the
    device table the draw kernels read.

    ``weights``: ``[num_posts]``.  A floating tensor must be finite, >= 0 and not all zero; it is
    quantised elementwise to integers, ``q = floor(w.double() / w.double().max() * (2^32 - 1))``,
    so a weight below ``max * 2^-32`` becomes 0 and that post is never drawn.  An integer tensor
    is taken as ``q`` itself (each in [0, 2^32), not all zero).  Post j is drawn with probability
    ``q[j] / T``, ``T = sum(q)``: draw c maps ``r = (splitmix64(seed + c * golden) * T) >> 64`` to
    the post with ``cdf[j] <= r < cdf[j + 1]`` (``cdf``: the exclusive sums of ``q``, int64, exact).

    It holds ``q``, ``cdf`` (``[num_posts + 1]``), ``T`` (read back once, here) and the guide table
    of the search: ``n_guide`` buckets of ``2^shift`` values of ``r`` each, as many buckets as
    posts (a power of two, at most 2^20: 4 MB beside 8 MB of cdf at 1M posts)."""

    GUIDE_MAX = 1 << 20

    def __init__(self, weights: torch.Tensor):
        if not isinstance(weights, torch.Tensor) or weights.dim() != 1 or weights.numel() < 1 or \
                weights.is_complex() or weights.dtype == torch.bool:
            raise ValueError("PostDistribution: weights must be a real [num_posts] tensor")
        if weights.numel() >= 2**31:
            raise ValueError("PostDistribution: num_posts must be below 2^31")
        if weights.is_floating_point():
            w = weights.detach().double()
            if not bool(torch.isfinite(w).all()):
                raise ValueError("PostDistribution: weights must be finite")
            if bool((w < 0).any()):
                raise ValueError("PostDistribution: weights must be >= 0")
            top = w.max()
            if float(top) == 0.0:
                raise ValueError("PostDistribution: weights are all zero")
            q = torch.floor(w / top * float(2**32 - 1)).to(torch.int64)
        else:
            q = weights.detach().to(torch.int64)
            if bool((q < 0).any()) or bool((q >= 2**32).any()):
                raise ValueError("PostDistribution: integer weights must lie in [0, 2^32)")
            if not bool((q > 0).any()):
                raise ValueError("PostDistribution: weights are all zero")
        dev = N.require_device(weights)
        lib, s = N.lib(), N.stream_ptr(dev)
        self.num_posts = int(q.numel())
        self.q = q.contiguous()
        self.cdf = torch.empty(self.num_posts + 1, dtype=torch.int64, device=dev)
        ws = N.workspace(lib.hgnn_weighted_cdf_ws_bytes(self.num_posts), dev)
        N.check(lib.hgnn_weighted_cdf_build(N.ptr(self.q), self.num_posts, N.ptr(self.cdf),
                                            N.ptr(ws), ws.numel(), s), "hgnn_weighted_cdf_build")
        self.T = int(self.cdf[-1])              # host sync: once per distribution
        gbits = min(max(self.num_posts - 1, 1).bit_length(), self.GUIDE_MAX.bit_length() - 1)
        self.n_guide = 1 << gbits
        self.shift = max((self.T - 1).bit_length() - gbits, 0)
        self.guide = torch.empty(self.n_guide + 1, dtype=torch.int32, device=dev)
        N.check(lib.hgnn_weighted_guide_build(N.ptr(self.cdf), self.num_posts, self.T, self.shift,
                                              self.n_guide, N.ptr(self.guide), s),
                "hgnn_weighted_guide_build")

    @classmethod
    def from_degree(cls, pos_edges: torch.Tensor, num_posts: int,
                    power: float = 0.75) -> "PostDistribution":
        """Posts in proportion to ``in_degree ** power`` over ``pos_edges`` (``[2, E]``, row 1 the
        posts): word2vec's unigram^0.75 negatives.  A post without a positive edge is never
        drawn."""
        deg = torch.bincount(pos_edges[1].to(torch.int64), minlength=int(num_posts))
        if deg.numel() != int(num_posts):
            raise ValueError(f"PostDistribution.from_degree: a post index of {num_posts} or more")
        return cls(deg.double() ** float(power))

    def log_q(self, num_neg: int = 1) -> torch.Tensor:
        """The logQ table of this distribution for ``num_neg`` negatives per positive edge, as
        the ``logq=`` of the loss entry points: fp32 ``[num_posts]`` on the distribution's device,
        ``log(num_neg * max(q[j], 1) / T)`` computed in float64 from ``q`` and ``T`` and then
        cast — NCE's ``log(k Q(p))``.  A post of weight 0 is never drawn as a negative but may be
        a positive, and ``log 0`` would make its logit infinite: it gets the offset of the
        smallest drawable weight (``q = 1``), so every entry is finite by construction.  One
        tensor per ``num_neg``, kept: the loss checks and casts a table once per tensor object,
        so asking again every step costs nothing."""
        k = _num_neg_value(num_neg)
        cache = self.__dict__.setdefault("_log_q", {})
        t = cache.get(k)
        if t is None:
            t = cache[k] = torch.log(self.q.clamp(min=1).double() * float(k)
                                     / float(self.T)).to(torch.float32)
        return t

    def _table_args(self):
        """cdf, n_posts, T, guide, shift, n_guide in ABI order."""
        return (N.ptr(self.cdf), self.num_posts, self.T, N.ptr(self.guide), self.shift,
                self.n_guide)


def _num_neg_value(num_neg: int) -> int:
    if int(num_neg) != num_neg or num_neg < 1:
        raise ValueError(f"num_neg={num_neg!r}; expected a whole number of at least 1 negative "
                         "per positive edge")
    return int(num_neg)


def _draw_count(E: int, num_neg: int) -> int:
    if E * num_neg >= 2**31 - 1:
        raise ValueError(f"{E} positive edges x num_neg={num_neg} reach the negatives sort's "
                         "limit of 2^31 - 1 pairs")
    return E * num_neg


def draw_negatives(pos_edges: torch.Tensor, num_posts: int,
                   generator: Optional[torch.Generator] = None,
                   num_neg: int = 1, *, distribution=None, avoid=None) -> NegativeDraw:
    """:func:`sample_negatives` without the materialised array: the seed only (one tiny device
    draw from ``generator``, no host sync).  ``edge_bce_loss(..., neg_order='user')`` takes it.
    ``num_neg`` = k > 1: E·k draws, shape ``(E, k)``.

    Uniform draws only: ``distribution`` / ``avoid`` raise ``ValueError``.  A ``NegativeDraw`` is
    drawn again in the two kernels that read it, and a table search plus a rejection loop would
    be paid twice there; :func:`sample_negatives` materialises the weighted draws instead."""
    if distribution is not None or avoid is not None:
        raise ValueError("draw_negatives: distribution / avoid are not drawn lazily (the search "
                         "and the rejection loop would run in both kernels that regenerate the "
                         "draws); use sample_negatives, which materialises them")
    num_neg = _num_neg_value(num_neg)
    dev = N.require_device(pos_edges)
    if num_posts < 1 or num_posts >= 2**31:
        raise ValueError(f"num_posts={num_posts} out of range")
    n = _draw_count(int(pos_edges.shape[1]), num_neg)
    seed = torch.randint(0, 2**62, (1,), device=dev, dtype=torch.int64, generator=generator)
    return NegativeDraw(seed, n, num_posts, num_neg)


def sample_negatives(pos_edges: torch.Tensor, num_posts: int,
                     generator: Optional[torch.Generator] = None,
                     num_neg: int = 1, *, distribution: Optional["PostDistribution"] = None,
                     avoid=None, max_tries: int = 4,
                     kept_seen: Optional[torch.Tensor] = None):
    """One uniform negative post per positive edge (train_gnn.py:272's ``torch.randint``), drawn
    directly in the user-grouped order: the draws are iid, so only their labels move.
    ``num_neg`` = k > 1: k per positive edge, ``[E, k]`` (row p the negatives of user-grouped
    position p); 1: ``[E]``.

    int32 draws from ``hgnn_uniform_i32`` (a counter-based generator seeded from ``generator``
    on the device, no host sync): in range by construction, so the loss sorts them without the
    int64 validation pass.  ``edge_bce_loss`` also takes int64 ``torch.randint`` negatives.

    ``distribution`` (a :class:`PostDistribution`): the draws follow it instead
    (``hgnn_weighted_i32``; draw p·k + j is negative j of position p).  ``avoid`` (a
    ``metrics.SeenIndex``): a draw that the position's user has seen is drawn again, up to
    ``max_tries`` attempts in all (``hgnn_weighted_avoid_i32``; attempt 0 is the draw without
    ``avoid``); when every attempt is seen the last is kept and ``kept_seen``, an optional
    one-element int64 device tensor, is incremented on the device.  ``avoid`` alone rejects
    uniform draws.  With either argument the result is a :class:`SkewedNegatives` (``.values``:
    the tensor), which the loss takes with ``neg_order="user"``; the positions are those of the
    cached ``relation_csr`` the loss uses.  Without them this is the function it was."""
    num_neg = _num_neg_value(num_neg)
    if distribution is not None or avoid is not None:
        return _sample_skewed(pos_edges, num_posts, generator, num_neg, distribution, avoid,
                              max_tries, kept_seen)
    dev = N.require_device(pos_edges)
    E = int(pos_edges.shape[1])
    out = torch.empty(E if num_neg == 1 else (E, num_neg), dtype=torch.int32, device=dev)
    if E == 0:
        return out
    if num_posts < 1 or num_posts >= 2**31:
        raise ValueError(f"num_posts={num_posts} out of range")
    n = _draw_count(E, num_neg)
    seed = torch.randint(0, 2**62, (1,), device=dev, dtype=torch.int64,
                         generator=generator)
    N.check(N.lib().hgnn_uniform_i32(N.ptr(seed), n, int(num_posts), N.ptr(out),
                                     N.stream_ptr(dev)), "hgnn_uniform_i32")
    return out


def _sample_skewed(pos_edges, num_posts: int, generator, num_neg: int, distribution, avoid,
                   max_tries: int, kept_seen) -> SkewedNegatives:
    """:func:`sample_negatives` with ``distribution`` and / or ``avoid``."""
    if distribution is not None and not isinstance(distribution, PostDistribution):
        raise ValueError("sample_negatives: distribution must be a PostDistribution")
    if int(max_tries) != max_tries or max_tries < 1:
        raise ValueError(f"sample_negatives: max_tries={max_tries!r}; at least 1 attempt")
    if num_posts < 1 or num_posts >= 2**31:
        raise ValueError(f"num_posts={num_posts} out of range")
    if distribution is not None and distribution.num_posts != int(num_posts):
        raise ValueError(f"sample_negatives: the distribution is over {distribution.num_posts} "
                         f"posts, num_posts={num_posts}")
    if avoid is not None and avoid.num_posts != int(num_posts):
        raise ValueError(f"sample_negatives: avoid indexes {avoid.num_posts} posts, "
                         f"num_posts={num_posts}")
    if kept_seen is not None and (avoid is None or kept_seen.dtype != torch.int64
                                  or kept_seen.numel() != 1):
        raise ValueError("sample_negatives: kept_seen is a one-element int64 tensor, with avoid")
    dev = N.require_device(pos_edges, kept_seen)
    E = int(pos_edges.shape[1])
    out = torch.empty(E if num_neg == 1 else (E, num_neg), dtype=torch.int32, device=dev)
    if E == 0:
        return SkewedNegatives(out)
    n = _draw_count(E, num_neg)
    lib, s = N.lib(), N.stream_ptr(dev)
    seed = torch.randint(0, 2**62, (1,), device=dev, dtype=torch.int64, generator=generator)
    table = (distribution._table_args() if distribution is not None
             else (None, int(num_posts), 0, None, 0, 0))
    if avoid is None:
        # per draw a seed-free counter in, 4 B out, and a few 8-B cdf entries from the caches
        with _timed("weighted_negatives", 4 * n):
            N.check(lib.hgnn_weighted_i32(N.ptr(seed), n, *table, N.ptr(out), s),
                    "hgnn_weighted_i32")
        return SkewedNegatives(out)
    csr = relation_csr_for_loss(pos_edges, avoid.num_users, num_posts)
    uop = _user_of_pos(csr)
    with _timed("weighted_negatives_avoid", (4 + 4) * n):
        N.check(lib.hgnn_weighted_avoid_i32(
            N.ptr(seed), n, num_neg, *table, N.ptr(uop), avoid.num_users, N.ptr(avoid.rowptr),
            N.ptr(avoid._col), int(max_tries), N.ptr(out), N.ptr(kept_seen), s),
            "hgnn_weighted_avoid_i32")
    return SkewedNegatives(out)


HARD_NEG_MAX_CANDIDATES = 64   # the selection keeps a position's taken columns in one 64-bit mask


def mine_hard_negatives(user_emb: torch.Tensor, post_emb: torch.Tensor, pos_edges: torch.Tensor,
                        candidates, num_neg: int = 1, *, row_dtype: str = "fp32",
                        short: Optional[torch.Tensor] = None,
                        check: bool = False) -> SkewedNegatives:
    """Hard (model-scored) negatives: of M candidate posts per positive edge, the ``num_neg`` = k
    that the current tables score highest against the edge's user (``hgnn_hard_negatives``: one
    wave per user, the M post rows streamed per edge, nothing but ids written — no ``[E, M, d]``
    gather exists anywhere).

    ``user_emb`` / ``post_emb``: the current tables, detached: no gradient flows, the result is
    ids.  ``row_dtype="bf16"`` scores ``rows_to_bf16`` copies (``d % 8 == 0``);
    ``torch.bfloat16`` tables may be given directly.  The default is "fp32" whatever
    ``HGNN_ROW_DTYPE`` says, as in ``evaluate``.

    ``candidates``: an int32 ``[E, M]`` (or ``[E]``) tensor in the user-grouped order of the cached
    ``relation_csr`` (what :func:`sample_negatives` draws), a :class:`SkewedNegatives` holding
    one, or a :class:`NegativeDraw` with ``num_neg=M`` (the pool is then drawn inside the kernel,
    the same values as its ``tensor()``).  ``1 <= k <= M <= 64``.

    Per position: pick r is the candidate of the greatest fp32 score that is in range, is not
    the position's own positive and is not a post picked before, the lowest column on equal
    scores (NaN counts as -inf); so a row holds distinct posts in descending score order.  Where
    no such candidate is left the pick is the lowest unpicked in-range column whatever it holds,
    else the positive itself, and ``short`` (an optional one-element int64 device tensor) is
    incremented on the device, like ``kept_seen``.  ``check=True`` reads back the count of
    out-of-range candidate ids and raises on any: the only host sync.  Deterministic.

    The result is a :class:`SkewedNegatives` (int32 ``[E]`` for k = 1, else ``[E, k]``), which
    :func:`edge_bce_loss` (``neg_order="user"``), :func:`edge_bce_loss_raw` and
    :func:`presort_negatives` take and route to the planned dP gather.  It depends on the edges
    and the tables' shapes only, so it may be reused over several steps.  Once mined the
    negatives no longer follow the distribution they were drawn from: a ``logq=`` table from
    ``dist.log_q`` does not correct for them."""
    who = "mine_hard_negatives"
    k = _num_neg_value(num_neg)
    if user_emb.dim() != 2 or post_emb.dim() != 2 or user_emb.shape[1] != post_emb.shape[1]:
        raise ValueError(f"{who}: user_emb {tuple(user_emb.shape)} and post_emb "
                         f"{tuple(post_emb.shape)} must be [n, d] tables of one width")
    nu, np_, d = int(user_emb.shape[0]), int(post_emb.shape[0]), int(user_emb.shape[1])
    E = int(pos_edges.shape[1])
    draw, cand = None, None
    if isinstance(candidates, NegativeDraw):
        draw = candidates
        M, rows = draw.num_neg, draw.n // draw.num_neg
        if draw.num_posts != np_:
            raise ValueError(f"{who}: candidates were drawn over {draw.num_posts} posts, post_emb "
                             f"has {np_}")
    else:
        cand = candidates.values if isinstance(candidates, SkewedNegatives) else candidates
        if not isinstance(cand, torch.Tensor) or cand.dtype != torch.int32 or \
                cand.dim() not in (1, 2):
            got = f"{cand.dtype} {tuple(cand.shape)}" if isinstance(cand, torch.Tensor) \
                else type(cand).__name__
            raise ValueError(f"{who}: candidates must be int32 [E, M] (or [E]) in the "
                             f"user-grouped order, got {got}; draw them with sample_negatives, or "
                             "reorder COO-ordered ids with negatives_in_user_order and cast them")
        M, rows = (1 if cand.dim() == 1 else int(cand.shape[1])), int(cand.shape[0])
    if rows != E:
        raise ValueError(f"{who}: candidates has {rows} rows for {E} positive edges")
    if M < 1 or M > HARD_NEG_MAX_CANDIDATES:
        raise ValueError(f"{who}: candidates holds M={M} per edge; 1 <= M <= "
                         f"{HARD_NEG_MAX_CANDIDATES}")
    if k > M:
        raise ValueError(f"{who}: num_neg={k} exceeds the M={M} candidates per edge")
    _draw_count(E, k)
    bf16 = user_emb.dtype == torch.bfloat16
    if bf16 != (post_emb.dtype == torch.bfloat16):
        raise ValueError(f"{who}: user_emb and post_emb must both be fp32 or both bfloat16")
    cast = _row_dtype_value(row_dtype, "row_dtype") == "bf16" and not bf16
    if (bf16 or cast) and d % 8:
        raise ValueError(f"{who}: row_dtype='bf16' needs d % 8 == 0, got d={d}")
    if d > 512:
        raise ValueError(f"{who}: d={d}; rows of at most 512 columns")
    if short is not None and (not isinstance(short, torch.Tensor) or short.dtype != torch.int64
                              or short.numel() != 1):
        raise ValueError(f"{who}: short is a one-element int64 tensor")
    dev = N.require_device(user_emb, post_emb, pos_edges, cand,
                           draw.seed if draw is not None else None, short)
    U, P = user_emb.detach(), post_emb.detach()
    if cast:
        U, P = rows_to_bf16(_check_f32(U, f"{who} user_emb")), \
            rows_to_bf16(_check_f32(P, f"{who} post_emb"))
    else:
        U, P = _check_table(U, f"{who} user_emb"), _check_table(P, f"{who} post_emb")
    out = torch.empty(E if k == 1 else (E, k), dtype=torch.int32, device=dev)
    if E == 0:
        return SkewedNegatives(out)
    if np_ < 1 or np_ >= 2**31 - 1:
        raise ValueError(f"{who}: post_emb has {np_} rows, out of range")
    ub = relation_csr_for_loss(pos_edges, nu, np_).bwd
    if cand is not None:
        cand = cand.contiguous()
    err = torch.empty(1, dtype=torch.int32, device=dev) if check else None
    entry = "hgnn_hard_negatives_bf16" if U.dtype == torch.bfloat16 else "hgnn_hard_negatives"
    # per position M candidate rows, M ids in (none when they are drawn here), its positive's id
    # and k ids out; per user its own row
    rb = _row_bytes(U)
    nbytes = E * (M * rb + (4 * M if cand is not None else 0) + 4 + 4 * k) + nu * rb
    with _timed("hard_negatives", nbytes):
        N.check(getattr(N.lib(), entry)(
            N.ptr(U), N.ptr(P), d, nu, np_, N.ptr(ub.rowptr), N.ptr(ub.col), N.ptr(cand),
            N.ptr(draw.seed if draw is not None else None), M, k, N.ptr(out), N.ptr(short),
            N.ptr(err), N.stream_ptr(dev)), entry)
    if check and int(err[0]):
        raise ValueError(f"{who}: candidate post id out of range")
    return SkewedNegatives(out)


# ----------------------------------------------------------------------------- composable ops
# Differentiable single-kernel ops, used where a fused layer does not apply (the partitioned
# multi-GPU path in parallel.py composes them around RCCL collectives).
class _GatherMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_src, csr: RelationCSR, bf16: bool = False):
        ctx.csr = csr
        if bf16:     # the shadow lives for this gather only; K2 below is the fp32 one
            return gather_mean(rows_to_bf16(x_src), csr)
        return gather_mean(x_src, csr)

    @staticmethod
    def backward(ctx, g):
        await_pending(g)     # the halo exchange's adjoint may still be in flight (parallel.py)
        if not ctx.needs_input_grad[0]:
            return None, None, None
        if ctx.csr.num_edges == 0:
            # a zero gradient, not None: a rank holding no edge of this relation still has to
            # reach the collective adjoints upstream (parallel.py's halo exchange)
            return g.new_zeros(ctx.csr.n_src, g.shape[1]), None, None
        return scatter_mean_bwd(g.contiguous(), ctx.csr), None, None


def mean_gather(x_src: torch.Tensor, csr: RelationCSR,
                row_dtype: Optional[str] = None) -> torch.Tensor:
    """Differentiable K1 (forward) / K2 (backward) mean aggregation.  ``row_dtype="bf16"``: the
    forward gathers the bf16 copy of ``x_src`` (a width that is no multiple of 8 keeps fp32
    rows); the backward is the same fp32 K2 either way, the gradient passing straight through the
    rounding.  None is "fp32" whatever ``ROW_DTYPE`` says: this is the composable op of the
    sharded path (parallel.py), which stays on fp32 rows."""
    bf16 = (row_dtype is not None and _row_dtype_value(row_dtype, "row_dtype") == "bf16"
            and x_src.dim() == 2 and x_src.shape[1] % 8 == 0)
    if not bf16:
        return _GatherMean.apply(x_src, csr)
    return _GatherMean.apply(x_src, csr, True)


# Gradients still being produced by an in-flight collective (parallel.py issues the adjoint of
# its post-table all-reduce asynchronously): the consumer below waits on the collective right
# before its first kernel, so the user-side backward kernels scheduled in between overlap it.
_PENDING: Dict[int, Tuple[torch.Tensor, object]] = {}


def defer_until(t: torch.Tensor, work) -> torch.Tensor:
    """Register ``t`` as not yet valid until ``work.wait()`` (a torch.distributed Work)."""
    _PENDING[id(t)] = (t, work)
    return t


def await_pending(t: torch.Tensor) -> torch.Tensor:
    entry = _PENDING.pop(id(t), None)
    if entry is not None and entry[0] is t:
        with torch.no_grad():
            entry[1].wait()   # NCCL: the current stream waits on the collective (no host sync)
    return t


def weighted_gather_raw(x_src: torch.Tensor, csr: RelationCSR, w_fwd: torch.Tensor,
                        row_w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[i] = sum_{p in row i} w_fwd[p] x_src[col[p]]`` (K1 with per-edge weights).
    ``row_w``: the same weights when they are constant per row (w_fwd[p] = row_w[i], the
    sharded step's 1/deg_global): a source table of several GB is then gathered in
    source-block passes scaled per row (see :func:`gather_blocks`)."""
    x_src = _check_f32(x_src, "weighted_gather")
    out = torch.empty(csr.n_dst, x_src.shape[1], dtype=torch.float32, device=x_src.device)
    B = gather_blocks(x_src, csr.num_edges) if (row_w is not None and csr.num_edges) else 1
    if B > 1:
        passes, _ = csr.blocks("fwd", B)
        d, E = int(x_src.shape[1]), csr.num_edges
        _gather_blocked(x_src, passes, row_w, None, out, False,
                        f"gather_wfwd[{csr.n_dst}<-{csr.n_src}]x{d}",
                        gather_bytes(E, csr.n_dst, d, False),
                        gather_compulsory_bytes(E, csr.n_dst, csr.n_src, d, False))
        return out
    _gather(x_src, csr.fwd, None, csr_mean=False, out=out, accumulate=False, edge_w=w_fwd,
            kind="wfwd")
    return out


def weighted_scatter_bwd_raw(g: torch.Tensor, csr: RelationCSR, w_bwd: torch.Tensor,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Transpose of :func:`weighted_gather_raw` over the CSC (K2), accumulating into ``out``."""
    acc = out is not None
    if out is None:
        out = torch.empty(csr.n_src, g.shape[1], dtype=torch.float32, device=g.device)
    _gather(g.contiguous(), csr.bwd, None, csr_mean=False, out=out, accumulate=acc, edge_w=w_bwd)
    return out


class _GatherWeighted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_src, csr: RelationCSR, w_fwd, w_bwd):
        x_src = _check_f32(x_src, "weighted_gather")
        out = torch.empty(csr.n_dst, x_src.shape[1], dtype=torch.float32, device=x_src.device)
        _gather(x_src, csr.fwd, None, csr_mean=False, out=out, accumulate=False, edge_w=w_fwd,
                kind="wfwd")
        ctx.csr, ctx.w_bwd = csr, w_bwd
        return out

    @staticmethod
    def backward(ctx, g):
        await_pending(g)
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        csr = ctx.csr
        if csr.num_edges == 0:   # zero, not None: see _GatherMean.backward
            return g.new_zeros(csr.n_src, g.shape[1]), None, None, None
        out = torch.empty(csr.n_src, g.shape[1], dtype=torch.float32, device=g.device)
        _gather(g.contiguous(), csr.bwd, None, csr_mean=False, out=out, accumulate=False,
                edge_w=ctx.w_bwd)
        return out, None, None, None


def weighted_gather(x_src: torch.Tensor, csr: RelationCSR, w_fwd: torch.Tensor,
                    w_bwd: torch.Tensor) -> torch.Tensor:
    """``out[i] = sum_{p in row i} w_fwd[p] x_src[col[p]]`` (CSR order weights); backward walks
    the CSC with ``w_bwd`` (CSC order) — the same edge weights, transposed."""
    return _GatherWeighted.apply(x_src, csr, w_fwd, w_bwd)


class _FusedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, relu: bool, w, b, *segs):
        segs = [_check_f32(s, "fused_linear") for s in segs]
        y = linear_fwd(segs, w.contiguous(), None if b is None else b.contiguous(), relu)
        ctx.relu, ctx.has_b = relu, b is not None
        ctx.save_for_backward(w, y, *segs)
        return y

    @staticmethod
    def backward(ctx, dy):
        await_pending(dy)    # a slice gradient whose reduce-scatter may be in flight (parallel.py)
        w, y, *segs = ctx.saved_tensors
        need = ctx.needs_input_grad
        dxs = [torch.empty_like(s) if need[3 + i] else None for i, s in enumerate(segs)]
        dw, db = linear_bwd(segs, w, dy.contiguous(), y if ctx.relu else None, dxs, need[1],
                            ctx.has_b and need[2])
        return (None, dw, db, *dxs)


def fused_linear(segs: Sequence[torch.Tensor], w: torch.Tensor, b: Optional[torch.Tensor],
                 relu: bool) -> torch.Tensor:
    """Differentiable K3: ``act(sum_s segs[s] @ w[:, seg s]^T + b)``."""
    return _FusedLinear.apply(relu, w, b, *segs)

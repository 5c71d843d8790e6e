"""Tensor-level wrappers over the C-ABI (include/g2v.h).  PyTorch is plumbing only: it owns device
memory and the stream; every number is produced by the HIP kernels in libg2v_hip.so.

All tensors must live on the GPU, be fp32 (uint8 masks, int64 indices, int32 lengths) and contiguous
unless a stride argument says otherwise.  Nothing here falls back to torch arithmetic."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import CodeDecGrads, CodeDecSaved, CodeDecWeights, DecGrads, DecSaved, DecWeights, check


def _lib_():
    return _lib.load()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype=torch.float32, name="tensor"):
    if not t.is_cuda:
        raise _lib.G2VLibraryError(f"{name} must be a GPU tensor: the g2v kernels have no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


# ---- side branches (round 6) ------------------------------------------------------------------------------------------------
# Part d's iteration is an autograd chain on ONE stream; a good part of its backward is weight-gradient work nothing downstream
# waits for (a layer's, while its input gradient moves on).
# Inside `with side_branches():` (train_iter_text2embedding, GraphedText2EmbeddingStep) a block under `with side_branch(k, keep)`
# is launched on side stream k, forked from the current stream; `join_side()` (FlatParams.gather_grads, and the scope's exit)
# makes the current stream wait for all of them.  Outside such a scope a side_branch block runs inline: somebody who calls
# backward() and reads .grad without an optimiser step never sees an unjoined stream.
#   * `keep`: every tensor the block READS that was allocated on the forking stream -- the caching allocator hands a block
#     back to its own stream's pool the moment the last reference dies (the end of the autograd node), while the side launch may
#     still be reading; they stay referenced until the join.  What the block ALLOCATES belongs to the side stream's pool and is
#     only ever recycled there, stream-ordered behind the fork.
#   * the reusable workspaces are per branch (a tag suffix): two weight-gradient launches on two streams never share slabs.
#   * a gradient produced on a side stream must not be ACCUMULATED into an existing .grad by autograd (an add on the main
#     stream); every parameter of Part d's model receives one contribution per iteration and zero_grad() resets to None.
import contextlib
import os
import threading

_side_state = {"active": 0, "streams": {}, "pending": []}
_side_local = threading.local()
SIDE_BRANCHES = os.environ.get("G2V_SIDE_BRANCHES", "1") != "0"


def join_side():
    """the current stream waits for every side branch forked since the last join (their kept tensors are released)"""
    pend, _side_state["pending"] = _side_state["pending"], []
    if pend:
        cur = torch.cuda.current_stream()
        for s, _keep in pend:
            cur.wait_stream(s)


def reset_side_streams():
    """Forget the cached side streams (new ones are drawn at the next fork).  GraphedText2EmbeddingStep does this in front of every
    capture: on ROCm 7.2 the replay of the FOURTH multi-stream graph captured over the same side streams in one process, with the
    third still alive, died inside hipGraphLaunch (gpurun_tools/r06_side_repro.py: seq4 against seq4fresh / seq4gc)."""
    join_side()
    _side_state["streams"].clear()


@contextlib.contextmanager
def side_branches(enabled: bool = True):
    on = bool(enabled) and SIDE_BRANCHES
    _side_state["active"] += 1 if on else 0
    try:
        yield
    finally:
        if on:
            _side_state["active"] -= 1
            join_side()


@contextlib.contextmanager
def side_branch(k: int = 0, keep=(), rows: int = 1 << 62, min_rows: int = 0):
    """rows / min_rows: the caller's size rule -- a fork costs two cross-queue edges of the replayed graph (5-10 us each) and the
    co-running kernels slow each other down; measured on Part d (gpurun_tools/r06_side_mask.py, profiles/r06_i_side_mask.log):
    the encoder's weight gradients beside its input-gradient chain pay from B = 2048 (-2 ... -4 %), cost 1-3 % at B = 1024 and
    10 % at B = 128 with attention; the decoder's parameter gradients beside the encoder's BPTT never paid and stay inline."""
    if not _side_state["active"] or rows < min_rows:
        yield False
        return
    cur = torch.cuda.current_stream()
    key = (cur.device.index, int(k))
    s = _side_state["streams"].get(key)
    if s is None:
        s = _side_state["streams"][key] = torch.cuda.Stream(device=cur.device)
    s.wait_stream(cur)
    prev = getattr(_side_local, "suffix", "")
    _side_local.suffix = f"@side{int(k)}"
    try:
        with torch.cuda.stream(s):
            yield True
    finally:
        _side_local.suffix = prev
        _side_state["pending"].append((s, keep))


_ws_cache = {}
_ws_retired = []      # superseded workspaces stay allocated: see workspace()


def workspace(nbytes: int, device, tag: str = "ws") -> torch.Tensor:
    """A reusable byte buffer per (device, tag); grows monotonically (allocation never happens inside the C-ABI).

    A buffer that is outgrown is RETIRED, never freed: its address may be baked into a captured hipGraph
    (train_eval.train_seq2seq.GraphedText2EmbeddingStep replays ops.* calls), and handing the block back to the caching
    allocator would let a later replay scribble its weight-gradient slabs over whatever tensor reuses the memory.  The cost
    is bounded: sizes only grow, so at most a geometric series of small blocks per tag stays behind."""
    key = (str(device), tag + getattr(_side_local, "suffix", ""))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        grow = max(int(nbytes), 256, 0 if buf is None else 2 * buf.numel())
        buf = torch.empty(grow, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# ------------------------------------------------------------------------------------------ linear
def linear_fwd(x, w, bias=None, act=0, *, M=None, ldx=None, row_map=None, keep=None, scale=1.0, out=None, ldy=None):
    """y = act(x w^T + b).  row_map = (rows_inner, stride_outer, stride_inner) in elements."""
    N, K = w.shape
    if M is None:
        M = x.numel() // K
    if ldx is None:
        ldx = K
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    if ldy is None:
        ldy = N
    ri, so, si = row_map if row_map is not None else (0, 0, 0)
    check(_lib_().g2v_linear_fwd(_p(x), ldx, ri, so, si, _p(keep), float(scale), _p(_chk(w, name="w")), _p(bias),
                                 _p(out), ldy, M, K, N, act, _stream()), "linear_fwd")
    return out


def linear_route(form, M, K, N, *, N_b=0, act=0, bias=True, keep=False, row_map=None, ldx=None, ldy=None, smallm_rows=-1,
                 unaligned=()) -> str:
    """g2v_linear_route as a name: "SMALLM*2" (tn = 2), "STREAM*12x4" (the (NTW, KS) instance), "K4", "K4*1" (row-mapped),
    "TILED*4" / "TILED*1" (float4 / scalar operands), "TILED*4|ONE_LAUNCH" (pair and dual forms: both products in one launch); ""
    where the call is refused.  form "FWD" / "BWD_DATA" / "FWD_PAIR" / "FWD_DUAL"; w is (N, K) in every form; ldx / ldy: row strides
    of the array read and written (default: dense); unaligned: names of the G2V_DENSE_ALIGN_* facts that do NOT hold (torch
    allocations are 16-byte aligned: none); smallm_rows -1: the bound context's."""
    c = _lib.CONSTANTS
    bwd = form == "BWD_DATA"
    ri, so, si = row_map if row_map is not None else (0, 0, 0)
    align = sum(v for k, v in c.items() if k.startswith("G2V_DENSE_ALIGN_") and k[len("G2V_DENSE_ALIGN_"):] not in unaligned)
    r = _lib_().g2v_linear_route(c["G2V_DENSE_FORM_" + form], int(M), int(K), int(N), int(N_b), int(act), int(bool(bias)), int(bool(keep)),
                                 int(ri), int(so), int(si), int((N if bwd else K) if ldx is None else ldx),
                                 int((K if bwd else N) if ldy is None else ldy), int(smallm_rows), align)
    names = {v: k[len("G2V_DENSE_ROUTE_"):] for k, v in c.items() if k.startswith("G2V_DENSE_ROUTE_")}
    route, v = names.get(r & 0xff, ""), (r >> 8) & 0xff
    variant = f"*{v >> 4}x{v & 15}" if route == "STREAM" else (f"*{v}" if v else "")
    return route + variant + ("|ONE_LAUNCH" if r & c["G2V_DENSE_ROUTE_ONE_LAUNCH"] else "")


def linear_compose2(w0, b0, w1, b1, w_in, b_in):
    """(w_p w_in, w_p b_in + b_p) for p = 0, 1 (g2v_linear_compose2): two linear layers in a row as one."""
    G, H = w0.shape
    D = w_in.shape[1]
    dev = w0.device
    wc = [torch.empty((G, D), dtype=torch.float32, device=dev) for _ in range(2)]
    bc = [torch.empty((G,), dtype=torch.float32, device=dev) for _ in range(2)]
    check(_lib_().g2v_linear_compose2(_p(_chk(w0, name="w0")), _p(b0), _p(_chk(w1, name="w1")), _p(b1), _p(_chk(w_in, name="w_in")),
                                      _p(b_in), _p(wc[0]), _p(bc[0]), _p(wc[1]), _p(bc[1]), G, H, D, _stream()), "linear_compose2")
    return wc[0], bc[0], wc[1], bc[1]


def linear_fwd_pair(x, w_a, bias_a, w_b, bias_b, act=0, *, M=None):
    """(act(x w_a^T + b_a), act(x w_b^T + b_b)) in one launch where that pays (g2v_linear_fwd_pair)."""
    N, K = w_a.shape
    if M is None:
        M = x.numel() // K
    ya = torch.empty((M, N), dtype=torch.float32, device=x.device)
    yb = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(_lib_().g2v_linear_fwd_pair(_p(x), K, _p(_chk(w_a, name="w_a")), _p(bias_a), _p(ya), _p(_chk(w_b, name="w_b")), _p(bias_b),
                                      _p(yb), N, M, K, N, act, _stream()), "linear_fwd_pair")
    return ya, yb


def linear_bwd_data(dy, w, *, M=None, lddy=None, out=None, lddx=None, accumulate=False):
    N, K = w.shape
    if M is None:
        M = dy.numel() // N
    if lddy is None:
        lddy = N
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    if lddx is None:
        lddx = K
    check(_lib_().g2v_linear_bwd_data(_p(dy), lddy, _p(w), _p(out), lddx, M, K, N, int(accumulate), _stream()),
          "linear_bwd_data")
    return out


def _wgrad_flags(accumulate, bf16x3=False) -> int:
    """the flag word of the g2v_linear_bwd_weight family (include/g2v.h G2V_WGRAD_*)"""
    return (_lib.WGRAD_ACCUMULATE if accumulate else 0) | (_lib.WGRAD_BF16X3 if bf16x3 else 0)


def wgrad_items(items):
    """[(dy, x, dw, db-or-None), ...] of one shape, as tensors or raw device addresses -> the g2v_wgrad_item array of the batch calls"""
    arr = (_lib.WgradItem * len(items))()
    for a, item in zip(arr, items):
        a.dy, a.x, a.dw, a.db = (v.data_ptr() if isinstance(v, torch.Tensor) else v for v in item)
    return arr


def linear_bwd_weight(dy, x, N, K, *, M=None, lddy=None, ldx=None, row_map=None, keep=None, scale=1.0,
                      dw=None, db=None, want_bias=True, accumulate=False, bf16x3=False):
    """dw = dy^T xin (+ db).  bf16x3=True allows the 3-term bf16 split products (G2V_WGRAD_BF16X3, ~1.5e-5 relative)."""
    if M is None:
        M = dy.numel() // N
    if lddy is None:
        lddy = N
    if ldx is None:
        ldx = K
    dev = dy.device
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dev)
    if db is None and want_bias:
        db = torch.empty((N,), dtype=torch.float32, device=dev)
    lib = _lib_()
    nbytes = lib.g2v_linear_bwd_weight_workspace(M, K, N)
    ws = workspace(nbytes, dev, "bwdw")
    ri, so, si = row_map if row_map is not None else (0, 0, 0)
    check(lib.g2v_linear_bwd_weight(_p(dy), lddy, _p(x), ldx, ri, so, si, _p(keep), float(scale), _p(dw), _p(db),
                                    M, K, N, _wgrad_flags(accumulate, bf16x3), _p(ws), ws.numel(), _stream()),
          "linear_bwd_weight")
    return dw, db


def linear_bwd_weight_sum2(dy_a, dy_b, x, N, K, *, M, lddy=None, ldx=None, row_map=None, dw=None, db=None, want_bias=True,
                           accumulate=False):
    """dw = (dy_a + dy_b)^T x (+ db) without the add pass; raises for shapes g2v_linear_bwd_weight_sum2_ok() rejects."""
    dev = dy_a.device
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dev)
    if db is None and want_bias:
        db = torch.empty((N,), dtype=torch.float32, device=dev)
    lib = _lib_()
    ws = workspace(lib.g2v_linear_bwd_weight_workspace(M, K, N), dev, "bwdw")
    ri, so, si = row_map if row_map is not None else (0, 0, 0)
    check(lib.g2v_linear_bwd_weight_sum2(_p(dy_a), _p(dy_b), lddy if lddy is not None else N, _p(x),
                                         ldx if ldx is not None else K, ri, so, si, _p(dw), _p(db), M, K, N,
                                         int(bool(accumulate)), _p(ws), ws.numel(), _stream()), "linear_bwd_weight_sum2")
    return dw, db


def linear_bwd_weight_batch(items, N, K, *, M, lddy=None, ldx=None, accumulate=False, bf16x3=False, row_map=None):
    """items: up to 4 tuples (dy, x, dw, db-or-None) of ONE shape -> one launch + one slab reduction (large M).
    row_map = (rows_inner, stride_outer, stride_inner): x row-mapped as in linear_fwd (g2v_linear_bwd_weight_batch_mapped)."""
    lib = _lib_()
    arr = wgrad_items(items)
    dev = items[0][0].device
    ws = workspace(len(items) * lib.g2v_linear_bwd_weight_workspace(M, K, N), dev, "bwdw")
    if row_map is not None:
        check(lib.g2v_linear_bwd_weight_batch_mapped(arr, len(items), lddy if lddy is not None else N, ldx if ldx is not None else K,
                                                     row_map[0], row_map[1], row_map[2], M, K, N,
                                                     _wgrad_flags(accumulate, bf16x3), _p(ws), ws.numel(), _stream()),
              "linear_bwd_weight_batch_mapped")
        return
    check(lib.g2v_linear_bwd_weight_batch(arr, len(items), lddy if lddy is not None else N, ldx if ldx is not None else K, M, K, N,
                                          _wgrad_flags(accumulate, bf16x3), _p(ws), ws.numel(), _stream()),
          "linear_bwd_weight_batch")


class WgradDeferred:
    """The slab reductions of several weight-gradient calls, held back and run as ONE launch (include/g2v.h:
    g2v_linear_bwd_weight_deferred / _reduce).  Every call gets a 256-byte-aligned region of `ws` of its own (its slabs live there
    until `flush`), `flush` reduces the pending records in chunks of G2V_WGRAD_PENDING_MAX.  Round 6: a chain of immediate calls
    made every product wait for the reduction of the one in front of it, and beside the encoder's BPTT kernel -- whose two
    workgroups per CU leave a late-dispatched kernel no registers -- those reductions took 17-95 us instead of 5
    (profiles/r05_az_step_timeline.txt: 133 us of them on the decoder branch's chain)."""

    def __init__(self, ws: torch.Tensor):
        self.ws, self.off, self.pend = ws, 0, []

    @staticmethod
    def region(nprob, M, K, N) -> int:
        return int(nprob * _lib_().g2v_linear_bwd_weight_workspace(M, K, N))

    def call(self, items, lddy, ldx, row_map, dy_b, M, K, N, flags) -> int:
        """items: a g2v_wgrad_item array (wgrad_items).  -> the record's nprob: 0 where the call completed dw / db itself"""
        need, off = self.region(len(items), M, K, N), self.off
        self.off = (off + need + 255) & ~255
        assert self.off <= self.ws.numel(), "deferred weight-gradient workspace too small"
        pd = _lib.WgradPending()
        check(_lib_().g2v_linear_bwd_weight_deferred(items, len(items), lddy, ldx, row_map[0], row_map[1], row_map[2], dy_b, M, K, N,
                                                     flags, self.ws.data_ptr() + off, need, C.byref(pd), _stream()),
              "linear_bwd_weight_deferred")
        self.pend.append(pd)
        return pd.nprob

    def flush(self):
        live = [p for p in self.pend if p.nprob > 0]
        self.pend, self.off = [], 0
        for k in range(0, len(live), _lib.WGRAD_PENDING_MAX):
            chunk = live[k:k + _lib.WGRAD_PENDING_MAX]
            check(_lib_().g2v_linear_bwd_weight_reduce((_lib.WgradPending * len(chunk))(*chunk), len(chunk), _stream()),
                  "linear_bwd_weight_reduce")


def linear_bwd_weight_deferred(calls, *, accumulate=False, bf16x3=False):
    """Several weight-gradient calls whose slab reductions run as ONE launch behind the last product (WgradDeferred).  calls: list
    of dicts {items: [(dy, x, dw, db-or-None), ...] of one shape, N, K, M, lddy, ldx, row_map, dy_b}.  Results are bitwise those
    of the immediate calls.  -> the pending problems per call (0: completed inside the call)."""
    dev = calls[0]["items"][0][0].device
    tot = sum((WgradDeferred.region(len(c["items"]), c["M"], c["K"], c["N"]) + 255) & ~255 for c in calls)
    dfr = WgradDeferred(workspace(tot + 256, dev, "bwdw_deferred"))
    nprob = [dfr.call(wgrad_items(c["items"]), c.get("lddy", c["N"]), c.get("ldx", c["K"]), c.get("row_map") or (0, 0, 0),
                      _p(c.get("dy_b")), c["M"], c["K"], c["N"], _wgrad_flags(accumulate, bf16x3)) for c in calls]
    dfr.flush()
    return nprob


def linear_bwd_weight_fold2(w0, w1, p0, p1, c0, c1, dw=None, db=None, accumulate=False):
    """dw = w0^T p0 + w1^T p1, db = w0^T c0 + w1^T c1 (g2v_linear_bwd_weight_fold2: the weight gradient of a layer in front of
    two parallel layers from their weight-gradient-shaped products).  w: (G,H), p: (G,D), c: (G) -> dw (H,D), db (H)."""
    G, H = w0.shape
    D = p0.shape[1]
    if dw is None:
        dw = torch.empty((H, D), dtype=torch.float32, device=w0.device)
    if db is None:
        db = torch.empty((H,), dtype=torch.float32, device=w0.device)
    check(_lib_().g2v_linear_bwd_weight_fold2(_p(_chk(w0, name="w0")), _p(_chk(w1, name="w1")), _p(p0), _p(p1), _p(c0), _p(c1),
                                              _p(dw), _p(db), G, H, D, int(bool(accumulate)), _stream()), "linear_bwd_weight_fold2")
    return dw, db


def linear_bwd_weight_chain2(p0, p1, c0, c1, w_in, b_in, accumulate=False, dw0=None, dw1=None):
    """dw_p = p_p w_in^T + c_p b_in^T (g2v_linear_bwd_weight_chain2).  p: (G,D), c: (G), w_in: (H,D), b_in: (H) -> two (G,H)."""
    G, D = p0.shape
    H = w_in.shape[0]
    if dw0 is None:
        dw0 = torch.empty((G, H), dtype=torch.float32, device=p0.device)
    if dw1 is None:
        dw1 = torch.empty((G, H), dtype=torch.float32, device=p0.device)
    check(_lib_().g2v_linear_bwd_weight_chain2(_p(p0), _p(p1), _p(c0), _p(c1), _p(_chk(w_in, name="w_in")), _p(b_in), _p(dw0), _p(dw1),
                                               G, H, D, int(bool(accumulate)), _stream()), "linear_bwd_weight_chain2")
    return dw0, dw1


def linear_bwd_weight_fold_chain2(w0, w1, p0, p1, c0, c1, w_in, b_in):
    """linear_bwd_weight_fold2 + linear_bwd_weight_chain2 in one launch -> (dw_in, db_in, dw0, dw1)."""
    G, H = w0.shape
    D = p0.shape[1]
    dev = w0.device
    dw_in, db_in = torch.empty((H, D), dtype=torch.float32, device=dev), torch.empty((H,), dtype=torch.float32, device=dev)
    dw0, dw1 = torch.empty((G, H), dtype=torch.float32, device=dev), torch.empty((G, H), dtype=torch.float32, device=dev)
    check(_lib_().g2v_linear_bwd_weight_fold_chain2(_p(_chk(w0, name="w0")), _p(_chk(w1, name="w1")), _p(p0), _p(p1), _p(c0), _p(c1),
                                                    _p(_chk(w_in, name="w_in")), _p(b_in), _p(dw_in), _p(db_in), _p(dw0), _p(dw1),
                                                    G, H, D, _stream()), "linear_bwd_weight_fold_chain2")
    return dw_in, db_in, dw0, dw1


# ------------------------------------------------------------------------------------------ quantiser
def vq_code_sqnorm(codebook, out=None):
    K, E = codebook.shape
    if out is None:
        out = torch.empty((K,), dtype=torch.float32, device=codebook.device)
    check(_lib_().g2v_vq_code_sqnorm(_p(_chk(codebook)), _p(out), K, E, _stream()), "vq_code_sqnorm")
    return out


def vq_route(form, wants, N, E, K, *, smallm_rows=-1, facts=()) -> str:
    """g2v_vq_assign_route as a name: "BX", "FUSED*1" (variant 1), "PACKED*4", "SPLIT*8", "PROJECT>PACKED*2" (pre_linear, then that
    route on the projected rows), ...; "" where the call is refused.  form "ROWS" / "RAW", wants "FULL" / "IDX" / "IDX_BULK", facts:
    names of G2V_VQ_PLAN_* bits; smallm_rows -1: the bound context's."""
    c = _lib.CONSTANTS
    r = _lib_().g2v_vq_assign_route(c["G2V_VQ_FORM_" + form], c["G2V_VQ_WANTS_" + wants], int(N), int(E), int(K), int(smallm_rows),
                                    sum(c["G2V_VQ_PLAN_" + f] for f in facts))
    names = {v: k[len("G2V_VQ_ROUTE_"):] for k, v in c.items() if k.startswith("G2V_VQ_ROUTE_")}
    one = lambda x: names.get(x & 0xff, "") + (f"*{(x >> 8) & 0xff}" if (x >> 8) & 0xff else "")
    return one(r) + (">" + one(r >> 16) if r >> 16 else "")


def vq_assign(flat, z, codebook, code_sqnorm, want_quantized=True, want_dist=False, route=None):
    """-> idx (N) int64, quantized (N,E) | None, dist_min (N) | None, sse_partial | None.  route: vq_route's answer for these rows,
    where the caller has asked already."""
    N, E = flat.shape
    K = codebook.shape[0]
    dev = flat.device
    lib = _lib_()
    idx = torch.empty((N,), dtype=torch.int64, device=dev)
    quant = torch.empty((N, E), dtype=torch.float32, device=dev) if want_quantized else None
    dmin = torch.empty((N,), dtype=torch.float32, device=dev) if want_dist else None
    sse = torch.empty((lib.g2v_vq_assign_blocks(N),), dtype=torch.float32, device=dev) if want_quantized else None
    if route is None:
        route = vq_route("ROWS", "FULL" if want_quantized else "IDX", N, E, K)
    if route.startswith("PACKED"):
        # the reference's own quantiser shapes (E = 400): fragment-major codebook image + the eight-wave kernel, same outputs bit
        # for bit (g2v_vq_assign_packed_fwd); the image is rebuilt per call (6 us: nothing is trusted across calls)
        frag = workspace(K * E * 4, flat.device, "vqpack").view(torch.float32)[:K * E]
        check(lib.g2v_vq_pack_codebook(_p(_chk(codebook)), _p(frag), K, E, _stream()), "vq_pack_codebook")
        check(lib.g2v_vq_assign_packed_fwd(_p(_chk(flat)), _p(z), _p(codebook), _p(frag), _p(code_sqnorm), _p(idx), _p(quant),
                                           _p(dmin), _p(sse), N, E, K, _stream()), "vq_assign_packed_fwd")
        return idx, quant, dmin, sse
    check(lib.g2v_vq_assign_fwd(_p(_chk(flat)), _p(z), _p(_chk(codebook)), _p(code_sqnorm), _p(idx), _p(quant),
                                _p(dmin), _p(sse), N, E, K, _stream()), "vq_assign_fwd")
    return idx, quant, dmin, sse


def vq_assign_raw(z, w_pre, b_pre, codebook):
    """Code indices (N) int64 from RAW latents: argmin_k |z w_pre^T + b_pre - W_k|^2 on the route g2v_vq_assign_route names for a
    caller that accepts the screened bulk kernels (they return the fp32 kernels' indices)."""
    N, E = z.shape
    K = codebook.shape[0]
    route = vq_route("RAW", "IDX_BULK", N, E, K)
    wsq = vq_code_sqnorm(codebook)
    if route == "BULK_Z":
        return vq_assign_bulk_z(z, w_pre, b_pre, codebook, wsq)
    flat = linear_fwd(z, w_pre, b_pre)
    rows = route.partition(">")[2]          # PROJECT>...; a refused call ("") gets its error from g2v_vq_assign_fwd
    if rows.startswith("BULK"):
        return vq_assign_bulk(flat, codebook, wsq)
    return vq_assign(flat, None, codebook, wsq, want_quantized=False, route=rows)[0]


def vq_assign_bulk(flat, codebook, code_sqnorm, want_undecided=False):
    """idx (N,) = argmin_k |flat - W_k|^2 for many rows: bf16 split screening + exact fp32 re-check (g2v_vq_assign_bulk)."""
    N, E = flat.shape
    K = codebook.shape[0]
    lib = _lib_()
    idx = torch.empty((N,), dtype=torch.int64, device=flat.device)
    nb = int(lib.g2v_vq_assign_bulk_workspace(N, E, K))
    ws = workspace(nb, flat.device, "vqbulk")
    und = torch.zeros((1,), dtype=torch.int32, device=flat.device) if want_undecided else None
    check(lib.g2v_vq_assign_bulk(_p(_chk(flat)), _p(_chk(codebook)), _p(_chk(code_sqnorm)), _p(idx), N, E, K, _p(ws), nb, _p(und),
                                 _stream()), "vq_assign_bulk")
    return (idx, und) if want_undecided else idx


def vq_assign_bulk_z_ok(N, E, K) -> bool:
    """shapes g2v_vq_assign_bulk_z serves (E = 400, K % 16 == 0, 32 <= K <= 512, N >= 2048 and above smallm_rows: the rows whose
    pre_linear product linear_route("FWD", N, 400, 400) names "TILED*4", the kernel whose bits it promises)"""
    return bool(_lib_().g2v_vq_assign_bulk_z_ok(int(N), int(E), int(K)))


def vq_assign_bulk_z(z, w_pre, b_pre, codebook, code_sqnorm, want_undecided=False):
    """idx (N,) = argmin_k |z w_pre^T + b_pre - W_k|^2 from RAW latents, bitwise linear_fwd + vq_assign at the same N:
    z-space bf16 screening + exact fp32 re-check (g2v_vq_assign_bulk_z); the projected rows are never written."""
    N, E = z.shape
    K = codebook.shape[0]
    lib = _lib_()
    idx = torch.empty((N,), dtype=torch.int64, device=z.device)
    nb = int(lib.g2v_vq_assign_bulk_z_workspace(N, E, K))
    ws = workspace(nb, z.device, "vqbulkz")
    und = torch.zeros((1,), dtype=torch.int32, device=z.device) if want_undecided else None
    check(lib.g2v_vq_assign_bulk_z(_p(_chk(z, name="z")), _p(_chk(w_pre, name="w_pre")), _p(_chk(b_pre, name="b_pre")),
                                   _p(_chk(codebook, name="codebook")), _p(_chk(code_sqnorm, name="code_sqnorm")), _p(idx), N, E, K,
                                   _p(ws), nb, _p(und), _stream()), "vq_assign_bulk_z")
    return (idx, und) if want_undecided else idx


def vq_pack_codebook(codebook, out=None):
    """fragment-major image of the codebook for vq_fused_assign(..., codebook_frag=)"""
    K, E = codebook.shape
    if out is None:
        out = torch.empty((K * E,), dtype=torch.float32, device=codebook.device)
    check(_lib_().g2v_vq_pack_codebook(_p(_chk(codebook)), _p(out), K, E, _stream()), "vq_pack_codebook")
    return out


def vq_fused_assign(z, w_pre, b_pre, codebook, code_sqnorm, codebook_frag=None):
    """pre_linear + assign in one launch (E == 128, K % 128 == 0) -> flat (N,E), idx (N) int64, quantized (N,E), sse_partial.
    codebook_frag (vq_pack_codebook): read the distance operands from the fragment-major image (same results, faster loads)."""
    N, E = z.shape
    K = codebook.shape[0]
    dev = z.device
    lib = _lib_()
    flat = torch.empty((N, E), dtype=torch.float32, device=dev)
    idx = torch.empty((N,), dtype=torch.int64, device=dev)
    quant = torch.empty((N, E), dtype=torch.float32, device=dev)
    sse = torch.empty((lib.g2v_vq_assign_blocks(N),), dtype=torch.float32, device=dev)
    if codebook_frag is not None:
        check(lib.g2v_vq_fused_assign_packed_fwd(_p(_chk(z)), _p(_chk(w_pre)), _p(_chk(b_pre)), _p(_chk(codebook)),
                                                 _p(_chk(codebook_frag)), _p(_chk(code_sqnorm)), _p(flat), _p(idx), _p(quant),
                                                 _p(sse), N, E, K, _stream()), "vq_fused_assign_packed_fwd")
        return flat, idx, quant, sse
    check(lib.g2v_vq_fused_assign_fwd(_p(_chk(z)), _p(_chk(w_pre)), _p(_chk(b_pre)), _p(_chk(codebook)), _p(_chk(code_sqnorm)),
                                      _p(flat), _p(idx), _p(quant), _p(sse), N, E, K, _stream()), "vq_fused_assign_fwd")
    return flat, idx, quant, sse


VQ_BX_EXACT = _lib.VQ_BX_EXACT          # include/g2v.h G2V_VQ_BX_*


def vq_bx_pack(codebook, code_sqnorm, w_pre, b_pre, out=None):
    """screening operands of vq_fused_assign_bx (g2v_vq_bx_pack): bf16 fragments of U = W w_pre, s'_k, per-code radius coefficients"""
    K, E = codebook.shape
    nb = int(_lib_().g2v_vq_bx_image_bytes(K, E))
    if out is None:
        out = torch.empty((nb,), dtype=torch.uint8, device=codebook.device)
    check(_lib_().g2v_vq_bx_pack(_p(_chk(codebook)), _p(_chk(code_sqnorm)), _p(_chk(w_pre)), _p(_chk(b_pre)), _p(out), K, E,
                                 _stream()), "vq_bx_pack")
    return out


def vq_fused_assign_bx(z, w_pre_frag, b_pre, codebook, image, code_sqnorm, flags=0, want_diag=False):
    """pre_linear + bf16-screened / fp32-re-checked assign in one launch (g2v_vq_fused_assign_bx_fwd) -> flat, idx, quantized,
    sse_partial[, diag int32[4]: tiles on the exact sweep, pairs re-evaluated].  w_pre_frag = vq_pack_codebook(w_pre)."""
    N, E = z.shape
    K = codebook.shape[0]
    dev = z.device
    lib = _lib_()
    flat = torch.empty((N, E), dtype=torch.float32, device=dev)
    idx = torch.empty((N,), dtype=torch.int64, device=dev)
    quant = torch.empty((N, E), dtype=torch.float32, device=dev)
    sse = torch.empty((lib.g2v_vq_assign_blocks(N),), dtype=torch.float32, device=dev)
    diag = torch.zeros((4,), dtype=torch.int32, device=dev) if want_diag else None
    check(lib.g2v_vq_fused_assign_bx_fwd(_p(_chk(z)), _p(_chk(w_pre_frag)), _p(_chk(b_pre)), _p(_chk(codebook)), _p(image),
                                         _p(_chk(code_sqnorm)), _p(flat), _p(idx), _p(quant), _p(sse), _p(diag), N, E, K,
                                         int(flags), _stream()), "vq_fused_assign_bx_fwd")
    return (flat, idx, quant, sse, diag) if want_diag else (flat, idx, quant, sse)


def vq_stats(idx, flat, K, out=None):
    N, E = flat.shape
    dev = flat.device
    lib = _lib_()
    if out is None:
        out = torch.empty((K + K * E,), dtype=torch.float32, device=dev)
    ws = workspace(lib.g2v_vq_stats_workspace(N, E, K), dev, "vqstats")
    check(lib.g2v_vq_stats(_p(_chk(idx, torch.int64)), _p(_chk(flat)), _p(out), N, E, K, _p(ws), ws.numel(),
                           _stream()), "vq_stats")
    return out


def vq_ema_update(stats, sse_partial, ema_cluster_size, ema_w, codebook, code_sqnorm, N_loss, N_cnt, E, K,
                  beta, decay, eps, update, scalars=None, exact_decay=False):
    """exact_decay: the weight of the new statistics is (float)(1.0 - decay) formed in double, as torch forms the reference's Python
    scalar (g2v_vq_ema_update_exact); otherwise 1.0f - (float)decay, what the chunk quantiser's path has always computed"""
    if scalars is None:
        scalars = torch.empty((2,), dtype=torch.float32, device=stats.device)
    fn = _lib_().g2v_vq_ema_update_exact if exact_decay else _lib_().g2v_vq_ema_update
    check(fn(_p(stats), _p(sse_partial), 0 if sse_partial is None else sse_partial.numel(),
             _p(ema_cluster_size), _p(ema_w), _p(codebook), _p(code_sqnorm), _p(scalars),
             N_loss, N_cnt, E, K, float(beta), float(decay), float(eps), int(update), _stream()), "vq_ema_update")
    return scalars


def vq_bwd(g_quantized, g_loss, z, codebook, idx, beta, out=None):
    """idx=None: `codebook` is the dense (N,E) saved `quantized` output."""
    N, E = z.shape
    gz = torch.empty_like(z) if out is None else out
    check(_lib_().g2v_vq_bwd(_p(g_quantized), _p(g_loss), _p(_chk(z)), _p(_chk(codebook)), _p(idx), _p(gz), N, E,
                             float(beta), _stream()), "vq_bwd")
    return gz


# ------------------------------------------------------------------------------------------ GRU direction(s)
def gru_packed_ok(T, B, H) -> bool:
    return bool(_lib_().g2v_gru_seq_packed_ok(int(T), int(B), int(H)))


def _row_off_array(row_off, T):
    """ctypes int32 array of the T packed row offsets (host memory: the library reads it at call time)"""
    if row_off is None:
        return None
    assert len(row_off) == T
    return (C.c_int32 * T)(*[int(v) for v in row_off])


def gru_gather_ok(T, B, H, ndir=2) -> bool:
    """g2v_gru_seq_fwd can gather its input projections from a table (g2v_gru_dir.gi_gather) for this shape"""
    return bool(_lib_().g2v_gru_seq_gather_ok(int(T), int(B), int(H), int(ndir)))


def gru_route(T, B, H, ndir=1, *, backward=False, cluster=-1, resident_rows=-1, resident_bwd=-1, cus=0, facts=()) -> str:
    """g2v_gru_seq_route as a name: "FAST", "FAST*1" (variant 1), "CLUSTER", "STEP", "RESIDENT", "STREAM", "STREAM*2", ...; "" where
    the call is refused.  facts: names of G2V_GRU_PLAN_* bits; -1 / cus=0: the bound context's options / the device's CU count."""
    r = _lib_().g2v_gru_seq_route(int(backward), int(T), int(B), int(H), int(ndir), int(cluster), int(resident_rows), int(resident_bwd),
                                  int(cus), sum(_lib.CONSTANTS["G2V_GRU_PLAN_" + f] for f in facts))
    name = {v: k[len("G2V_GRU_ROUTE_"):] for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_GRU_ROUTE_")}.get(r & 0xff, "")
    return name + (f"*{r >> 8}" if r >> 8 else "")


def code_route(S1, B, H, K, Tw=0, att=False, *, backward=False, layers=2, fused_min_rows=0, persistent=-1, cus=0, facts=()) -> str:
    """g2v_attn_code_rollout_route as a name: "CLUSTER", "STEP", "STEP*1" (variant 1: a launch per step), "CHAIN"; "" where the call
    is refused.  backward: False / True, or 2 for g2v_code_cluster_bptt called by itself; facts: names of G2V_CODE_PLAN_* bits;
    -1 / cus=0: the bound context's level / the device's CU count."""
    r = _lib_().g2v_attn_code_rollout_route(int(backward), int(S1), int(B), int(H), int(K), int(Tw), int(bool(att)), int(layers),
                                            int(fused_min_rows), int(persistent), int(cus),
                                            sum(_lib.CONSTANTS["G2V_CODE_PLAN_" + f] for f in facts))
    name = {v: k[len("G2V_CODE_ROUTE_"):] for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_CODE_ROUTE_")}.get(r & 0xff, "")
    return name + (f"*{r >> 8}" if r >> 8 else "")


def gru_dirs_fwd(dirs, T, B, H, *, lengths=None, hs_ld=None, row_off=None):
    """dirs: list (1 or 2) of dicts gi, w_hh, b_hh, h0, hs, h_n, gates, reverse -- ONE launch for both directions.
    With gi=None and x, w_ih, b_ih, in_dim given the input projection is fused into the kernel (H == in_dim == 64).
    row_off (T ints): gi is PACKED -- row (t,b) at row_off[t] + b, only positions inside their sequences (g2v.h)."""
    lib = _lib_()
    arr = (_lib.GruDir * len(dirs))()
    ro = _row_off_array(row_off, T)
    for k, d in enumerate(dirs):
        for name in ("gi", "w_hh", "b_hh", "h0", "hs", "h_n", "gates", "x", "w_ih", "b_ih", "gi_gather"):
            setattr(arr[k], name, _p(d.get(name)))
        arr[k].reverse = int(bool(d.get("reverse", False)))
        arr[k].in_dim = int(d.get("in_dim", 0))
        if ro is not None:
            arr[k].gi_row_off = ro
    dev = dirs[0]["hs"].device
    ws = workspace(lib.g2v_gru_seq_fwd_workspace(len(dirs), H), dev, "grufwd")
    check(lib.g2v_gru_seq_fwd(arr, len(dirs), _p(lengths), hs_ld if hs_ld is not None else H, T, B, H, _p(ws),
                              ws.numel(), _stream()), "gru_seq_fwd")


def side_pending() -> bool:
    """True while a side branch forked in this iteration has not been joined (its launches may still be running)"""
    return bool(_side_state["pending"])


def gru_dirs_bwd(dirs, T, B, H, *, lengths=None, d_hs_ld=None, hs_ld=None, row_off=None, allow_resident=True):
    """dirs: list of dicts d_hs, d_hn, hs, h0, gates, w_hh, dgi, dgh, dh0, reverse.  row_off: dgi is PACKED (see gru_dirs_fwd).
    allow_resident=False: this call keeps the streaming BPTT whatever G2V_OPT_GRU_RESIDENT_BWD says (a W_hh-resident launch takes
    every CU whole: a caller with other launches in flight beside it says so)."""
    lib = _lib_()
    arr = (_lib.GruDirBwd * len(dirs))()
    ro = _row_off_array(row_off, T)
    for k, d in enumerate(dirs):
        if ro is not None:
            arr[k].dgi_row_off = ro
        for name in ("d_hs", "d_hn", "hs", "h0", "gates", "w_hh", "dgi", "dgh", "dh0", "w_ih", "dx",
                     "x", "dw_hh", "db_hh", "dw_ih", "db_ih", "wslab"):        # the last six: optional fused weight gradients
            setattr(arr[k], name, _p(d.get(name)))
        arr[k].reverse = int(bool(d.get("reverse", False)))
        arr[k].in_dim = int(d.get("in_dim", 0))
    dev = dirs[0]["hs"].device
    ws = workspace(lib.g2v_gru_seq_bwd_workspace(len(dirs), H), dev, "grubwd")
    with contextlib.nullcontext() if allow_resident else _lib.Context.current().scoped(gru_resident_bwd=0):
        check(lib.g2v_gru_seq_bwd(arr, len(dirs), _p(lengths), d_hs_ld if d_hs_ld is not None else H,
                                  hs_ld if hs_ld is not None else H, T, B, H, _p(ws), ws.numel(), _stream()), "gru_seq_bwd")


def gru_seq_fwd(gi, w_hh, b_hh, T, B, H, *, h0=None, lengths=None, reverse=False, hs=None, hs_ld=None,
                save_gates=True):
    dev = gi.device
    if hs is None:
        hs = torch.empty((T, B, H), dtype=torch.float32, device=dev)
        hs_ld = H
    h_n = torch.empty((B, H), dtype=torch.float32, device=dev)
    gates = torch.empty((T, B, 4 * H), dtype=torch.float32, device=dev) if save_gates else None
    gru_dirs_fwd([dict(gi=_chk(gi), w_hh=_chk(w_hh), b_hh=b_hh, h0=h0, hs=hs, h_n=h_n, gates=gates, reverse=reverse)],
                 T, B, H, lengths=lengths, hs_ld=hs_ld)
    return hs, h_n, gates


def gru_seq_bwd(d_hs, d_hs_ld, d_hn, hs, hs_ld, h0, gates, w_hh, T, B, H, *, lengths=None, reverse=False,
                want_dh0=False):
    dev = hs.device
    dgi = torch.empty((T, B, 3 * H), dtype=torch.float32, device=dev)
    dgh = torch.empty((T, B, 3 * H), dtype=torch.float32, device=dev)
    dh0 = torch.empty((B, H), dtype=torch.float32, device=dev) if want_dh0 else None
    gru_dirs_bwd([dict(d_hs=d_hs, d_hn=d_hn, hs=hs, h0=h0, gates=gates, w_hh=w_hh, dgi=dgi, dgh=dgh, dh0=dh0,
                       reverse=reverse)], T, B, H, lengths=lengths, d_hs_ld=d_hs_ld, hs_ld=hs_ld)
    return dgi, dgh, dh0


def gru_cell_ok(in_dim, H, B):
    """shapes served by the one-launch GRU cell (small batch, generic hidden size)"""
    return in_dim % 4 == 0 and H % 4 == 0 and in_dim <= 256 and H <= 256 and B <= 1024


def gru_cell_fwd(x, h_prev, w_ih, w_hh, b_ih, b_hh, *, keep=None, scale=1.0, h_new=None, gates=None):
    """One GRU cell step incl. its input projection (g2v_gru_cell_fwd): x (B,in), h_prev (B,H) -> h_new (B,H), gates (B,4H)."""
    B, in_dim = x.shape
    H = h_prev.shape[1]
    if h_new is None:
        h_new = torch.empty((B, H), dtype=torch.float32, device=x.device)
    check(_lib_().g2v_gru_cell_fwd(_p(_chk(x)), in_dim, _p(keep), float(scale), _p(_chk(h_prev)), _p(_chk(w_ih)), _p(_chk(w_hh)),
                                   _p(b_ih), _p(b_hh), _p(h_new), _p(gates), B, H, _stream()), "gru_cell_fwd")
    return h_new


def gru_cell_bwd(d_h_a, d_h_b, gates, h_prev, w_ih, w_hh, *, keep=None, scale=1.0, dgi, dgh, d_hprev, dx=None):
    """Backward of gru_cell_fwd (g2v_gru_cell_bwd): fills dgi, dgh (B,3H), d_hprev (B,H), dx (B,in) [masked by keep * scale]."""
    B, H = h_prev.shape
    in_dim = w_ih.shape[1]
    check(_lib_().g2v_gru_cell_bwd(_p(d_h_a), _p(d_h_b), _p(_chk(gates)), _p(_chk(h_prev)), _p(_chk(w_ih)), _p(_chk(w_hh)), _p(keep),
                                   float(scale), _p(dgi), _p(dgh), _p(d_hprev), _p(dx), in_dim, B, H, _stream()), "gru_cell_bwd")


# ------------------------------------------------------------------------------------------ decoder rollout
def dec_weights_struct(wd: dict) -> DecWeights:
    s = DecWeights()
    for name, _ in DecWeights._fields_:
        setattr(s, name, _p(wd[name]))
    return s


def struct_from(cls, d: dict):
    """ctypes struct from a dict of tensors; array fields (e.g. DecGrads.dw_gru) take a list of tensors / None entries"""
    s = cls()
    for name, typ in cls._fields_:
        v = d.get(name)
        if isinstance(typ, type) and issubclass(typ, C.Array):
            for k, t in enumerate(v or ()):
                getattr(s, name)[k] = _p(t)
        else:
            setattr(s, name, _p(v))
    return s


def dec_rollout_blocks(B):
    return _lib_().g2v_dec_rollout_blocks(B)


def dec_rollout_fwd(target, h_init, wstruct, saved: dict, keep95, keep_l0, p_drop, n_pre, conditioned, training,
                    T, B, D, H):
    sv = struct_from(DecSaved, saved)
    lib = _lib_()
    ws = workspace(lib.g2v_dec_rollout_fwd_workspace(D, H), target.device, "decfwd")
    check(lib.g2v_dec_rollout_fwd(_p(_chk(target)), _p(_chk(h_init)), C.byref(wstruct), C.byref(sv),
                                  _p(_chk(keep95, torch.uint8)), _p(keep_l0), float(p_drop), int(n_pre),
                                  int(conditioned), int(training), T, B, D, H, _p(ws), ws.numel(), _stream()),
          "dec_rollout_fwd")


def dec_rollout_bwd(wstruct, saved: dict, grads: dict, keep95, keep_l0, p_drop, n_pre, conditioned, T, B, D, H):
    lib = _lib_()
    sv = struct_from(DecSaved, saved)
    gr = struct_from(DecGrads, grads)
    ws = workspace(lib.g2v_dec_rollout_bwd_workspace(D, H), grads["dy"].device, "decbwd")
    check(lib.g2v_dec_rollout_bwd(C.byref(wstruct), C.byref(sv), C.byref(gr), _p(keep95), _p(keep_l0),
                                  float(p_drop), int(n_pre), int(conditioned), T, B, D, H, _p(ws), ws.numel(),
                                  _stream()), "dec_rollout_bwd")


def bn_running_update(bn_stats, running_mean, running_var, steps, H, B):
    """Deferred commit of BatchNorm's running statistics from the bn_stats (steps,2,H) of a TRAINING rollout that was given
    bn_running_mean = bn_running_var = NULL; a no-op on the device while the persistent kernels' fault latch is set (include/g2v.h)."""
    check(_lib_().g2v_bn_running_update(_p(_chk(bn_stats)), _p(_chk(running_mean)), _p(_chk(running_var)), int(steps), int(H), int(B),
                                        _stream()), "bn_running_update")


# ------------------------------------------------------------------------------------------ Part d: fused code-decoder rollout
def code_cluster_bptt(dh_top, weights: dict, saved: dict, keep_l0, p_drop, S1, B, H, out=None):
    """g2v_code_cluster_bptt: the GRU cells' BPTT of the attention-free rollout as one persistent cluster launch (small batch).
    Returns (dgi0, dgh0, dgi1, dgh1 (S1,B,3H), da (S1,B,H), d_hidden0 (2,B,H)); out: these six, the caller's own arrays."""
    lib = _lib_()
    dev = dh_top.device
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    if out is not None:
        dgi0, dgh0, dgi1, dgh1, da, d_h0 = out
    else:
        dgi0, dgh0, dgi1, dgh1 = f32(S1, B, 3 * H), f32(S1, B, 3 * H), f32(S1, B, 3 * H), f32(S1, B, 3 * H)
        da, d_h0 = f32(S1, B, H), f32(2, B, H)
    ws = workspace(lib.g2v_code_cluster_bptt_workspace(B, H), dev, "codebptt")
    check(lib.g2v_code_cluster_bptt(_p(_chk(dh_top)), C.byref(struct_from(CodeDecWeights, weights)), C.byref(struct_from(CodeDecSaved, saved)),
                                    _p(keep_l0), float(p_drop), _p(dgi0), _p(dgh0), _p(dgi1), _p(dgh1), _p(da), _p(d_h0), S1, B, H,
                                    _p(ws), ws.numel(), _stream()), "code_cluster_bptt")
    return dgi0, dgh0, dgi1, dgh1, da, d_h0


def code_rollout_fwd(codes, h_init, enc, enc_proj, weights: dict, saved: dict, keep_emb, keep_l0, p_drop, n_pre, training,
                     S1, B, H, K, Tw):
    """g2v_attn_code_rollout_fwd: S1 + 1 launches of the fused decoder-step kernel (weights / saved: dicts of tensors named as
    the fields of g2v_code_dec_weights / g2v_code_dec_saved; missing = NULL)."""
    lib = _lib_()
    att = weights.get("w_attn") is not None
    ws = workspace(lib.g2v_attn_code_rollout_fwd_workspace(H, K, int(att)), h_init.device, "codefwd")
    check(lib.g2v_attn_code_rollout_fwd(_p(_chk(codes, torch.int64)), _p(_chk(h_init)), _p(enc), _p(enc_proj),
                                        C.byref(struct_from(CodeDecWeights, weights)), C.byref(struct_from(CodeDecSaved, saved)),
                                        _p(keep_emb), _p(keep_l0), float(p_drop), int(n_pre), int(training), S1, B, H, K, int(Tw),
                                        _p(ws), ws.numel(), _stream()), "attn_code_rollout_fwd")


def code_rollout_bwd(d_logits, enc, enc_proj, weights: dict, saved: dict, grads: dict, keep_emb, keep_l0, p_drop, S1, B, H, K, Tw):
    lib = _lib_()
    att = weights.get("w_attn") is not None
    ws = workspace(lib.g2v_attn_code_rollout_bwd_workspace(S1, B, H, K, int(Tw), int(att)), d_logits.device, "codebwd")
    check(lib.g2v_attn_code_rollout_bwd(_p(_chk(d_logits)), _p(enc), _p(enc_proj), C.byref(struct_from(CodeDecWeights, weights)),
                                        C.byref(struct_from(CodeDecSaved, saved)), C.byref(struct_from(CodeDecGrads, grads)),
                                        _p(keep_emb), _p(keep_l0), float(p_drop), S1, B, H, K, int(Tw), _p(ws), ws.numel(),
                                        _stream()), "attn_code_rollout_bwd")


# ------------------------------------------------------------------------------------------ Part d on continuous latents
def latent_rollout_ok(S1, B, H, E, att) -> bool:
    return bool(_lib_().g2v_latent_rollout_ok(int(S1), int(B), int(H), int(E), int(bool(att))))


def latent_rollout_fwd(target, h_init, weights: dict, saved: dict, keep_l0, p_drop, n_pre, S1, B, H, E):
    """g2v_latent_rollout_fwd: S1 + 1 launches of the fused decoder-step kernel of the continuous mode (weights / saved: dicts of
    tensors named as the fields of g2v_code_dec_weights / g2v_code_dec_saved with K := E; missing = NULL)."""
    lib = _lib_()
    ws = workspace(lib.g2v_latent_rollout_fwd_workspace(H, E), h_init.device, "latfwd")
    check(lib.g2v_latent_rollout_fwd(_p(_chk(target)), _p(_chk(h_init)), C.byref(struct_from(CodeDecWeights, weights)),
                                     C.byref(struct_from(CodeDecSaved, saved)), _p(keep_l0), float(p_drop), int(n_pre), S1, B, H, E,
                                     _p(ws), ws.numel(), _stream()), "latent_rollout_fwd")


def latent_rollout_bwd(d_out, weights: dict, saved: dict, grads: dict, keep_l0, p_drop, n_pre, S1, B, H, E):
    lib = _lib_()
    ws = workspace(lib.g2v_latent_rollout_bwd_workspace(S1, B, H, E), d_out.device, "latbwd")
    check(lib.g2v_latent_rollout_bwd(_p(_chk(d_out)), C.byref(struct_from(CodeDecWeights, weights)),
                                     C.byref(struct_from(CodeDecSaved, saved)), C.byref(struct_from(CodeDecGrads, grads)),
                                     _p(keep_l0), float(p_drop), int(n_pre), S1, B, H, E, _p(ws), ws.numel(), _stream()),
          "latent_rollout_bwd")


# ------------------------------------------------------------------------------------------ the text -> pose baseline (Seq2SeqNet)
def pose_attn_rollout_ok(S1, B, H, D, Tw) -> bool:
    return bool(_lib_().g2v_pose_attn_rollout_ok(int(S1), int(B), int(H), int(D), int(Tw)))


def pose_attn_rollout_plan(S1, B, H, D, Tw, fused_min_rows) -> int:
    """g2v_pose_attn_rollout_plan: 0 the per-operator chain, 1 the fused step kernels (host arithmetic only)."""
    return int(_lib_().g2v_pose_attn_rollout_plan(int(S1), int(B), int(H), int(D), int(Tw), int(min(fused_min_rows, 2 ** 31 - 1))))


def pose_attn_ldec(H, D) -> int:
    """Row stride of the saved input rows [x | c] (include/g2v.h: g2v_pose_attn_rollout_fwd)."""
    return (D + H + 3) & ~3


def pose_attn_rollout_fwd(target, h_init, enc, enc_proj, weights: dict, saved: dict, keep_l0, p_drop, n_pre, S1, B, H, D, Tw,
                          workspace_bytes=None):
    """g2v_pose_attn_rollout_fwd: S1 + 1 launches of the fused decoder-step kernel of the attention decoder with continuous
    feedback (weights / saved: dicts of tensors named as the fields of g2v_code_dec_weights / g2v_code_dec_saved with K := D;
    missing = NULL).  workspace_bytes: what the entry is told it has (tests of the refusal)."""
    lib = _lib_()
    ws = workspace(lib.g2v_pose_attn_rollout_fwd_workspace(H, D), h_init.device, "posefwd")
    check(lib.g2v_pose_attn_rollout_fwd(_p(target), _p(h_init), _p(enc), _p(enc_proj), C.byref(struct_from(CodeDecWeights, weights)),
                                        C.byref(struct_from(CodeDecSaved, saved)), _p(keep_l0), float(p_drop), int(n_pre), S1, B, H, D,
                                        int(Tw), _p(ws), ws.numel() if workspace_bytes is None else int(workspace_bytes), _stream()),
          "pose_attn_rollout_fwd")


def pose_attn_rollout_bwd(d_out, enc, enc_proj, weights: dict, saved: dict, grads: dict, keep_l0, p_drop, n_pre, S1, B, H, D, Tw):
    lib = _lib_()
    ws = workspace(lib.g2v_pose_attn_rollout_bwd_workspace(S1, B, H, D, int(Tw)), d_out.device, "posebwd")
    check(lib.g2v_pose_attn_rollout_bwd(_p(_chk(d_out)), _p(enc), _p(enc_proj), C.byref(struct_from(CodeDecWeights, weights)),
                                        C.byref(struct_from(CodeDecSaved, saved)), C.byref(struct_from(CodeDecGrads, grads)),
                                        _p(keep_l0), float(p_drop), int(n_pre), S1, B, H, D, int(Tw), _p(ws), ws.numel(), _stream()),
          "pose_attn_rollout_bwd")


# ------------------------------------------------------------------------------------------ loss / optimiser / rng
def custom_loss_fwd_bwd(y_tbd, target_btd, w_l1, w_cont, w_var, g_scale=1.0, want_grad=True):
    T, B, D = y_tbd.shape
    dev = y_tbd.device
    lib = _lib_()
    dy = torch.empty_like(y_tbd) if want_grad else None
    terms = torch.empty((5,), dtype=torch.float32, device=dev)
    partial = torch.empty((lib.g2v_custom_loss_blocks(B, D) * 4,), dtype=torch.float32, device=dev)
    check(lib.g2v_custom_loss_fwd_bwd(_p(_chk(y_tbd)), _p(_chk(target_btd)), _p(dy), _p(terms), _p(partial),
                                      float(w_l1), float(w_cont), float(w_var), float(g_scale), T, B, D, _stream()),
          "custom_loss_fwd_bwd")
    return terms, dy


def clip_adam_step(param, grad, m, v, step_counter, partial, gnorm_out, max_norm, grad_scale, lr, b1, b2, eps):
    check(_lib_().g2v_clip_adam_step(_p(_chk(param)), _p(_chk(grad)), _p(m), _p(v), param.numel(), _p(partial),
                                     _p(step_counter), _p(gnorm_out), float(max_norm), float(grad_scale), float(lr),
                                     float(b1), float(b2), float(eps), _stream()), "clip_adam_step")


def adam_blocks(n):
    return _lib_().g2v_adam_blocks(n)


def keep_mask(out_u8, keep_prob, seed, offset_counter):
    check(_lib_().g2v_keep_mask(_p(_chk(out_u8, torch.uint8)), out_u8.numel(), float(keep_prob), int(seed),
                                _p(offset_counter), _stream()), "keep_mask")
    return out_u8


def keep_mask_at(out_u8, keep_prob, seed, offset_counter, offset_add):
    """the mask keep_mask would draw after `offset_add` earlier draws, without bumping the counter (counter_add does, once)"""
    check(_lib_().g2v_keep_mask_at(_p(_chk(out_u8, torch.uint8)), out_u8.numel(), float(keep_prob), int(seed),
                                   _p(offset_counter), int(offset_add), _stream()), "keep_mask_at")
    return out_u8


def counter_add(counter, n):
    check(_lib_().g2v_counter_add(_p(_chk(counter, torch.int64)), int(n), _stream()), "counter_add")


def fill(t, v):
    check(_lib_().g2v_fill_f32(_p(t), float(v), t.numel(), _stream()), "fill")
    return t


def add_halves(a, lda, b, ldb, out, ldo, M, H):
    check(_lib_().g2v_add_halves(_p(a), lda, _p(b), ldb, _p(out), ldo, M, H, _stream()), "add_halves")
    return out


def scale(inp, scalar_dev, out=None):
    if out is None:
        out = torch.empty_like(inp)
    check(_lib_().g2v_scale_f32(_p(_chk(inp)), _p(scalar_dev), _p(out), inp.numel(), _stream()), "scale")
    return out


def mse_fwd_bwd(y, target, want_grad=True, g_scale=1.0, dy_out=None):
    """dy_out: a contiguous buffer of y's size for the gradient (a slice of a larger array, say)"""
    lib = _lib_()
    n = y.numel()
    dy = (dy_out if dy_out is not None else torch.empty_like(y)) if want_grad else None
    if dy is not None:
        _chk(dy, name="dy_out")
    loss = torch.empty((1,), dtype=torch.float32, device=y.device)
    partial = torch.empty((lib.g2v_mse_blocks(n),), dtype=torch.float32, device=y.device)
    check(lib.g2v_mse_fwd_bwd(_p(_chk(y)), _p(_chk(target)), _p(dy), _p(loss), _p(partial), n, float(g_scale), _stream()),
          "mse_fwd_bwd")
    return loss, dy


def vq_codebook_grad(stats, codebook, g_loss, N):
    K, E = codebook.shape
    out = torch.empty_like(codebook)
    check(_lib_().g2v_vq_codebook_grad(_p(stats), _p(_chk(codebook)), _p(g_loss), _p(out), N, E, K, _stream()),
          "vq_codebook_grad")
    return out


def mask_mul(inp, mask, scale=1.0, positive_of=False, out=None):
    """out = inp * scale where the mask is on (uint8 keep mask, or `mask > 0` for a float tensor when positive_of);
    out may be inp (elementwise)."""
    if out is None:
        out = torch.empty_like(inp)
    keep = None if positive_of else mask
    pos = mask if positive_of else None
    check(_lib_().g2v_mask_mul(_p(_chk(inp)), _p(keep), _p(pos), float(scale), _p(out), inp.numel(), _stream()), "mask_mul")
    return out


# ------------------------------------------------------------------------------------------ Part d operators
def embedding_fwd(table, ids, keep=None, scale=1.0, out=None, ldo=None):
    V, dim = table.shape
    n = ids.numel()
    if out is None:
        out, ldo = torch.empty((n, dim), dtype=torch.float32, device=table.device), dim
    check(_lib_().g2v_embedding_fwd(_p(_chk(table)), _p(_chk(ids, torch.int64)), _p(keep), float(scale), out.data_ptr(),
                                    ldo if ldo is not None else dim, n, dim, V, _stream()), "embedding_fwd")
    return out


def embedding_bwd(d_out, ids, V, keep=None, scale=1.0, reuse_sort=False):
    """reuse_sort: the PREVIOUS embedding_bwd call on this stream had the same ids, n, V and dim (its sort is still in the workspace)"""
    n, dim = d_out.shape
    d_table = torch.empty((V, dim), dtype=torch.float32, device=d_out.device)
    nb = int(_lib_().g2v_embedding_bwd_ws_bytes(n, dim, V))
    ws = workspace(nb, d_out.device, "embedding_bwd")
    check(_lib_().g2v_embedding_bwd(_p(_chk(d_out)), _p(_chk(ids, torch.int64)), _p(keep), float(scale), _p(d_table), n, dim,
                                    V, 1 | (2 if reuse_sort else 0), _p(ws), nb, _stream()), "embedding_bwd")
    return d_table


def batchnorm_fwd(x, weight, bias, running_mean, running_var, training, relu=True, out=None, save=None):
    """out: y buffer; save: (save_mean, save_invstd) buffers (training)"""
    B, H = x.shape
    y = torch.empty_like(x) if out is None else out
    if save is not None:
        sm, si = save
    else:
        sm = torch.empty((H,), dtype=torch.float32, device=x.device) if training else None
        si = torch.empty((H,), dtype=torch.float32, device=x.device) if training else None
    check(_lib_().g2v_batchnorm_fwd(_p(_chk(x)), _p(weight), _p(bias), _p(running_mean), _p(running_var), int(training),
                                    int(relu), _p(y), _p(sm), _p(si), B, H, _stream()), "batchnorm_fwd")
    return y, sm, si


def bn_running_update_invstd(save_mean, save_invstd, step_stride, running_mean, running_var, steps, H, B):
    """Deferred commit of BatchNorm's running statistics from the saved (mean, invstd) of `steps` training calls that were given
    no running statistics; a no-op on the device while the persistent kernels' fault latch is set (include/g2v.h)."""
    check(_lib_().g2v_bn_running_update_invstd(_p(save_mean), _p(save_invstd), int(step_stride), _p(running_mean), _p(running_var),
                                               int(steps), int(H), int(B), _stream()), "bn_running_update_invstd")


def batchnorm_bwd_steps(dy, x, y, weight, save_mean, save_invstd, relu=True):
    """BatchNorm's backward of the `steps` calls of a decode loop in one launch: dy, x, y (steps,B,H), save_* (steps,H) ->
    dx (steps,B,H) and the parameters' gradients summed over the steps (include/g2v.h: g2v_batchnorm_bwd_steps; B < 1024)."""
    S, B, H = x.shape
    dx = torch.empty_like(x)
    dw = torch.empty((H,), dtype=torch.float32, device=x.device)
    db = torch.empty((H,), dtype=torch.float32, device=x.device)
    if save_mean.stride(1) != 1 or save_invstd.stride(1) != 1 or save_mean.stride(0) != save_invstd.stride(0):
        raise ValueError("save_mean / save_invstd: rows of H contiguous floats at one common row stride")
    check(_lib_().g2v_batchnorm_bwd_steps(_p(_chk(dy)), _p(_chk(x)), _p(_chk(y)), _p(weight), _p(save_mean), _p(save_invstd),
                                          int(save_mean.stride(0)), int(relu), _p(dx), _p(dw), _p(db), S, B, H, _stream()),
          "batchnorm_bwd_steps")
    return dx, dw, db


def one_hot_rows(ids, K, out):
    """out[r, :] = one_hot(ids[r]) (float32; out a (M,K) view with contiguous rows)"""
    check(_lib_().g2v_one_hot_rows(_p(_chk(ids, torch.int64)), _p(out), int(out.stride(0)), int(ids.numel()), int(K), _stream()),
          "one_hot_rows")
    return out


def batchnorm_bwd(dy, x, y, weight, save_mean, save_invstd, relu=True, out=None):
    """out: (dx, dw, db) buffers"""
    B, H = x.shape
    if out is not None:
        dx, dw, db = out
    else:
        dx = torch.empty_like(x)
        dw = torch.empty((H,), dtype=torch.float32, device=x.device)
        db = torch.empty((H,), dtype=torch.float32, device=x.device)
    check(_lib_().g2v_batchnorm_bwd(_p(_chk(dy)), _p(x), _p(y), _p(weight), _p(save_mean), _p(save_invstd), int(relu), _p(dx),
                                    _p(dw), _p(db), B, H, _stream()), "batchnorm_bwd")
    return dx, dw, db


def cross_entropy_fwd_bwd(logits, targets, want_grad=True, ld=None, dl_out=None):
    M, K = logits.shape
    dev = logits.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    row = torch.empty((M,), dtype=torch.float32, device=dev)
    dl = (dl_out if dl_out is not None else torch.empty((M, K), dtype=torch.float32, device=dev)) if want_grad else None
    if dl is not None and (tuple(dl.shape) != (M, K) or not dl.is_contiguous()):
        raise ValueError("cross_entropy: dl_out must be a contiguous (M, K) array")
    check(_lib_().g2v_cross_entropy_fwd_bwd(_p(logits), ld if ld is not None else K, _p(_chk(targets, torch.int64)), _p(loss),
                                            _p(row), _p(dl), K, M, K, 1.0, _stream()), "cross_entropy")
    return loss, dl


def argmax_rows(x, out=None):
    M, K = x.shape
    if out is None:
        out = torch.empty((M,), dtype=torch.int64, device=x.device)
    check(_lib_().g2v_argmax_rows(_p(_chk(x)), K, _p(out), M, K, _stream()), "argmax_rows")
    return out


def attn_fwd(hp, ep, enc, v, ctx_out=None, ldctx=None, weights=None):
    """Bahdanau attention step: hp (B,H), ep/enc (T,B,H), v (H) -> weights (B,T), context (B,H) (optionally written
    into `ctx_out` with row stride ldctx, e.g. the second half of the decoder's (B,2H) input)."""
    T, B, H = enc.shape
    if weights is None:
        weights = torch.empty((B, T), dtype=torch.float32, device=enc.device)
    if ctx_out is None:
        ctx_out, ldctx = torch.empty((B, H), dtype=torch.float32, device=enc.device), H
    check(_lib_().g2v_attn_fwd(_p(_chk(hp)), _p(_chk(ep)), _p(_chk(enc)), _p(_chk(v)), _p(weights), ctx_out.data_ptr(),
                               ldctx, T, B, H, _stream()), "attn_fwd")
    return weights, ctx_out


def attn_step_fwd(logits, ids, table, keep, emb_scale, ec, hp, ep, enc, v, weights):
    """The row-local head of a decode step in one launch (include/g2v.h: g2v_attn_step_fwd): ids[b] = argmax(logits[b]) (logits
    None: ids given), ec[b, :H] = table[ids[b]] * keep * emb_scale, ec[b, H:] = attention context, weights (B,T)."""
    T, B, H = enc.shape
    K = table.shape[0]
    check(_lib_().g2v_attn_step_fwd(_p(logits), int(logits.stride(0)) if logits is not None else 0, K, _p(_chk(ids, torch.int64)),
                                    _p(_chk(table)), _p(keep), float(emb_scale), _p(ec), int(ec.stride(0)), _p(_chk(hp)), _p(_chk(ep)),
                                    _p(_chk(enc)), _p(_chk(v)), _p(weights), T, B, H, _stream()), "attn_step_fwd")


def slab_sum(slabs, out, accumulate=False):
    """out (+)= slabs.sum(0) in slab order (slabs (n, ...) contiguous)"""
    n = slabs.shape[0]
    check(_lib_().g2v_slab_sum(_p(_chk(slabs)), n, slabs.numel() // n, _p(out), int(bool(accumulate)), _stream()), "slab_sum")
    return out


def linear_fwd_dual(x, w_a, bias_a, out_a, w_b, bias_b, out_b):
    """out_a = x w_a^T + bias_a, out_b = x w_b^T + bias_b: one launch at small row counts (include/g2v.h: g2v_linear_fwd_dual)"""
    M, K = x.shape
    check(_lib_().g2v_linear_fwd_dual(_p(x), int(x.stride(0)), _p(_chk(w_a, name="w_a")), _p(bias_a), _p(out_a), int(out_a.stride(0)),
                                      w_a.shape[0], _p(_chk(w_b, name="w_b")), _p(bias_b), _p(out_b), int(out_b.stride(0)),
                                      w_b.shape[0], M, K, _stream()), "linear_fwd_dual")


def attn_bwd(d_ctx, hp, ep, enc, v, weights, ldd=None, out=None, accumulate=False, dv_slab=None):
    """out: (d_hp, d_ep, d_enc, d_v) buffers; accumulate adds into d_ep / d_enc / d_v (d_hp is always overwritten).
    dv_slab (B,H): d_v's per-row partials go there and stay unsummed (d_v is not touched: the caller sums the steps' slabs once)."""
    T, B, H = enc.shape
    dev = enc.device
    if out is not None:
        d_hp, d_ep, d_enc, d_v = out
    else:
        d_hp = torch.empty((B, H), dtype=torch.float32, device=dev)
        d_ep = torch.empty((T, B, H), dtype=torch.float32, device=dev)
        d_enc = torch.empty((T, B, H), dtype=torch.float32, device=dev)
        d_v = torch.empty((H,), dtype=torch.float32, device=dev)
    if dv_slab is not None:
        check(_lib_().g2v_attn_bwd(d_ctx.data_ptr(), ldd if ldd is not None else H, _p(hp), _p(ep), _p(enc), _p(v), _p(weights),
                                   _p(d_hp), _p(d_ep), _p(d_enc), None, int(bool(accumulate)), T, B, H, _p(_chk(dv_slab)),
                                   dv_slab.numel() * 4, _stream()), "attn_bwd")
        return d_hp, d_ep, d_enc, d_v
    nb = _lib_().g2v_attn_bwd_workspace(B, H)
    ws = workspace(nb, dev, "attn")
    check(_lib_().g2v_attn_bwd(d_ctx.data_ptr(), ldd if ldd is not None else H, _p(hp), _p(ep), _p(enc), _p(v), _p(weights),
                               _p(d_hp), _p(d_ep), _p(d_enc), _p(d_v), int(bool(accumulate)), T, B, H, _p(ws), ws.numel(),
                               _stream()), "attn_bwd")
    return d_hp, d_ep, d_enc, d_v


# ------------------------------------------------------------------------------------------ soft quantiser (GSSoft)
def vq_soft_fwd(flat, dots, logvar, wsq, want_perplexity=True):
    """dots (N,K) = flat W^T is overwritten with the squared distances; returns (probs (N,K), dist, perplexity (1,))."""
    N, E = flat.shape
    K = dots.shape[1]
    probs = torch.empty((N, K), dtype=torch.float32, device=flat.device)
    perp = torch.empty((1,), dtype=torch.float32, device=flat.device) if want_perplexity else None
    check(_lib_().g2v_vq_soft_fwd(_p(_chk(flat)), _p(_chk(dots)), _p(_chk(logvar)), _p(_chk(wsq)), _p(probs), None, N, E, K,
                                  _stream()), "vq_soft_fwd")
    if want_perplexity:        # its own device-wide pair of launches (the one built into g2v_vq_soft_fwd is a single workgroup)
        ws = torch.empty(int(_lib_().g2v_vq_soft_perplexity_workspace(N, K)), dtype=torch.uint8, device=flat.device)
        check(_lib_().g2v_vq_soft_perplexity(_p(probs), _p(perp), N, K, _p(ws), ws.numel(), _stream()), "vq_soft_perplexity")
    return probs, dots, perp


def vq_soft_bwd(probs, dprobs, dist, logvar):
    N, K = probs.shape
    dd = torch.empty_like(probs)
    dlv = torch.empty_like(probs)
    rowsum = torch.empty((N,), dtype=torch.float32, device=probs.device)
    check(_lib_().g2v_vq_soft_bwd(_p(_chk(probs)), _p(_chk(dprobs)), _p(_chk(dist)), _p(_chk(logvar)), _p(dd), _p(dlv), _p(rowsum),
                                  N, K, _stream()), "vq_soft_bwd")
    return dd, dlv, rowsum


def vq_soft_fused_ok(N, E, K):
    return bool(_lib_().g2v_vq_soft_fused_ok(N, E, K))


def vq_soft_fused_fwd(x, w_mean, b_mean, w_logvar, b_logvar, codebook, beta, g_scale=1.0, want_perplexity=True):
    """The whole soft-quantiser forward (csrc/vq_soft.hip): returns a dict flat, logvar, dist, probs, q, dq, quant, mse (1,),
    loss_vq (1,), perplexity (1,) or None."""
    lib = _lib_()
    N, E = x.shape
    K = codebook.shape[0]
    dev = x.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    wsq = vq_code_sqnorm(codebook)
    nblk = lib.g2v_vq_soft_fused_blocks(N)
    o = {"flat": f(N, E), "logvar": f(N, K), "dist": f(N, K), "probs": f(N, K), "q": f(N, E), "dq": f(N, E), "quant": f(N, E),
         "mse": f(1), "loss_vq": f(1), "perplexity": f(1) if want_perplexity else None}
    part, colsum = f(nblk), f(nblk, K) if want_perplexity else None
    check(lib.g2v_vq_soft_fused_fwd(_p(_chk(x)), _p(_chk(w_mean)), _p(_chk(b_mean)), _p(_chk(w_logvar)), _p(_chk(b_logvar)),
                                    _p(_chk(codebook)), _p(wsq), _p(o["flat"]), _p(o["logvar"]), _p(o["dist"]), _p(o["probs"]),
                                    _p(o["q"]), _p(o["dq"]), _p(o["quant"]), _p(part), _p(colsum), float(g_scale), N, E, K, _stream()),
          "vq_soft_fused_fwd")
    opb = torch.full((1,), 1.0 + float(beta), dtype=torch.float32, device=dev)
    check(lib.g2v_vq_soft_finish(_p(part), _p(colsum), _p(opb), _p(o["mse"]), _p(o["loss_vq"]), _p(o["perplexity"]), N, E, K,
                                 _stream()), "vq_soft_finish")
    return o


def vq_soft_fused_bwd(dh, g_loss, x, fwd, w_mean, w_logvar, codebook, beta):
    """Backward of vq_soft_fused_fwd (`fwd` = its dict): returns (gz (N,E), dd (N,K), dlogvar (N,K), dflat (N,E))."""
    N, E = x.shape
    K = codebook.shape[0]
    gz, dflat = torch.empty_like(x), torch.empty_like(x)
    dd, dlv = torch.empty_like(fwd["probs"]), torch.empty_like(fwd["probs"])
    check(_lib_().g2v_vq_soft_fused_bwd(_p(dh), _p(g_loss), _p(_chk(x)), _p(fwd["q"]), _p(fwd["dq"]), _p(fwd["flat"]), _p(fwd["probs"]),
                                        _p(fwd["dist"]), _p(fwd["logvar"]), _p(_chk(w_mean)), _p(_chk(w_logvar)), _p(_chk(codebook)),
                                        _p(dd), _p(dlv), _p(dflat), _p(gz), float(beta), N, E, K, _stream()), "vq_soft_fused_bwd")
    return gz, dd, dlv, dflat


def vae_latent_ok(B, E) -> bool:
    return bool(_lib_().g2v_vae_latent_ok(B, E))


def vae_latent_fwd(h, w_mean, b_mean, w_std, b_std, w_dec=None, b_dec=None, *, eps=None, seed=0, offset_counter=None,
                   sample=True, want_hf=True):
    """The variational block's forward (csrc/vae_latent.hip) on h (L,B,H): returns a dict mean, logvar, z (B,E), eps (B,E: the
    noise used -- `eps` itself when given, the drawn one otherwise; None with sample=False), hf (B,E) or None, d (L,B,H) or None
    (no w_dec), kl (1,).  Noise is drawn from the Philox stream (seed, offset_counter: device int64, advanced by 1) unless `eps`
    is given; sample=False gives z = mean."""
    lib = _lib_()
    L, B, H = h.shape
    E = L * H
    dev = h.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    draw = bool(sample) and eps is None
    o = {"mean": f(B, E), "logvar": f(B, E), "z": f(B, E), "eps": (f(B, E) if draw else eps) if sample else None,
         "hf": f(B, E) if want_hf else None, "d": f(L, B, H) if w_dec is not None else None, "kl": f(1)}
    ws = f(max(int(lib.g2v_vae_latent_fwd_workspace(B, E)) // 4, 4))
    check(lib.g2v_vae_latent_fwd(_p(_chk(h, name="h")), _p(_chk(w_mean, name="w_mean")), _p(_chk(b_mean, name="b_mean")),
                                 _p(_chk(w_std, name="w_std")), _p(_chk(b_std, name="b_std")),
                                 _p(_chk(w_dec, name="w_dec")) if w_dec is not None else None,
                                 _p(_chk(b_dec, name="b_dec")) if b_dec is not None else None,
                                 _p(_chk(eps, name="eps")) if eps is not None else None, int(seed), _p(offset_counter), int(bool(sample)),
                                 _p(o["mean"]), _p(o["logvar"]), _p(o["z"]), _p(o["eps"]) if draw else None, _p(o["hf"]), _p(o["d"]),
                                 _p(o["kl"]), _p(ws), ws.numel() * 4, B, L, H, _stream()), "vae_latent_fwd")
    return o


def vae_latent_bwd(g_d, g_kl, mean, logvar, eps, w_mean, w_std, w_dec, g_mean=None, g_logvar=None):
    """Backward of vae_latent_fwd: g_d (L,B,H) = d loss / d d, g_kl = device scalar d loss / d kl or None (0), eps None when the
    forward did not sample, g_mean / g_logvar (B,E) = gradients reaching mean / logvar directly or None
    -> (dh (L,B,H), dmean (B,E), dlogvar (B,E))."""
    L, B, H = g_d.shape
    dh = torch.empty_like(g_d)
    dmean, dlogvar = torch.empty_like(mean), torch.empty_like(mean)
    check(_lib_().g2v_vae_latent_bwd(_p(_chk(g_d, name="g_d")), _p(g_kl), _p(_chk(g_mean)) if g_mean is not None else None,
                                     _p(_chk(g_logvar)) if g_logvar is not None else None, _p(_chk(mean)), _p(_chk(logvar)),
                                     _p(_chk(eps, name="eps")) if eps is not None else None, _p(_chk(w_mean)), _p(_chk(w_std)),
                                     _p(_chk(w_dec)), _p(dmean), _p(dlogvar), _p(dh), B, L, H, _stream()), "vae_latent_bwd")
    return dh, dmean, dlogvar


def rowscale_combine(a, v, t):
    """out[r,c] = 2 a[r,c] v[r] - 2 t[r,c]"""
    rows, cols = a.shape
    out = torch.empty_like(a)
    check(_lib_().g2v_rowscale_combine(_p(_chk(a)), _p(_chk(v)), _p(_chk(t)), _p(out), rows, cols, _stream()), "rowscale_combine")
    return out


def ste(z, q):
    out = torch.empty_like(z)
    check(_lib_().g2v_ste_f32(_p(_chk(z)), _p(_chk(q)), _p(out), z.numel(), _stream()), "ste")
    return out


# ------------------------------------------------------------------------------------------ evaluation statistics
def moments_accumulate(x, shift, s1, s2, *, ld=None):
    """s1 (E,) f64 += sum_n (x_n - shift), s2 (E,E) f64 += sum_n (x_n - shift)(x_n - shift)^T over the rows of x (N,E) fp32 with row
    stride ld (g2v_moments_accumulate: fp32 MFMA on the upper triangle, mirrored; deterministic, additive for one shift)."""
    N, E = x.shape
    if not x.is_cuda:
        raise _lib.G2VLibraryError("x must be a GPU tensor: the g2v kernels have no CPU path")
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("moments_accumulate: x must be fp32 with unit column stride")
    ld = int(x.stride(0) if ld is None else ld)
    lib = _lib_()
    nb = int(lib.g2v_moments_workspace(N, E))
    ws = workspace(nb, x.device, "moments")
    check(lib.g2v_moments_accumulate(_p(x), ld, _p(_chk(shift, name="shift")), _p(_chk(s1, torch.float64, "s1")),
                                     _p(_chk(s2, torch.float64, "s2")), N, E, _p(ws), nb, _stream()), "moments_accumulate")
    return s1, s2


def code_histogram(idx, K, counts=None):
    """counts (K+1,) int64 += histogram of the code ids idx (N,) int64; ids outside [0, K) land in counts[K] (g2v_code_histogram)."""
    if counts is None:
        counts = torch.zeros((K + 1,), dtype=torch.int64, device=idx.device)
    check(_lib_().g2v_code_histogram(_p(_chk(idx, torch.int64, "idx")), idx.numel(), int(K), _p(_chk(counts, torch.int64, "counts")),
                                     _stream()), "code_histogram")
    return counts


NGRAM_MAX_LEN, NGRAM_MAX_K, NGRAM_MAX_N = 4096, 65536, 4        # the limits of g2v_ngram_clipped_counts (include/g2v.h)


def ngram_clipped_counts(cand, cand_start, cand_len, ref, ref_start, ref_len, K, max_n=4, max_len=NGRAM_MAX_LEN):
    """-> (clipped (B, max_n) int64, bad (1,) int64) of B (candidate, reference) pairs of code-id sequences (g2v_ngram_clipped_counts):
    clipped[b, n-1] = sum over candidate b's distinct n-grams of min(count in the candidate, count in the reference).  cand / ref: flat
    int64 id arrays; sequence b is the *_len[b] ids from element *_start[b] on (all (B,) int64, on the device, not read back).  max_len:
    the caller's upper bound on every length (it picks the kernel: give the tightest one known).  A pair with an id outside [0, K) or a
    length outside [0, max_len] has -1 in its row and counts in bad[0]."""
    B = cand_start.numel()
    for name, t in (("cand_len", cand_len), ("ref_start", ref_start), ("ref_len", ref_len)):
        if t.numel() != B:
            raise ValueError(f"ngram_clipped_counts: {name} has {t.numel()} entries, cand_start has {B}")
    if cand.numel() == 0 or ref.numel() == 0:                      # (every length on that side is 0: nothing is read, but the
        pad = torch.zeros((1,), dtype=torch.int64, device=cand.device)     # entry refuses a null pointer)
        cand, ref = (pad if cand.numel() == 0 else cand), (pad if ref.numel() == 0 else ref)
    clipped = torch.empty((B, int(max_n)), dtype=torch.int64, device=cand.device)
    bad = torch.zeros((1,), dtype=torch.int64, device=cand.device)
    i64 = torch.int64
    check(_lib_().g2v_ngram_clipped_counts(_p(_chk(cand, i64, "cand")), _p(_chk(cand_start, i64, "cand_start")),
                                           _p(_chk(cand_len, i64, "cand_len")), _p(_chk(ref, i64, "ref")),
                                           _p(_chk(ref_start, i64, "ref_start")), _p(_chk(ref_len, i64, "ref_len")), _p(clipped), _p(bad),
                                           B, int(K), int(max_n), int(max_len), _stream()), "ngram_clipped_counts")
    return clipped, bad


# ------------------------------------------------------------------------------------------ joint angles (clip_angles.hip)
ROT_METHODS = {"markley": _lib.ROT_MARKLEY, "procrustes": _lib.ROT_PROCRUSTES}


def rotmat_to_euler(frames, J, method, out=None, bad=None):
    """-> (angles (N, 3 J) degrees, bad (1,) int64) of frames (N, 9 J): per joint the intrinsic "ZXY" angles of its row-major 3x3
    matrix (g2v_rotmat_to_euler); method: ROT_METHODS' values.  A matrix whose determinant is not > 0 has NaN in its three angles and
    counts in bad[0], which is ADDED to (a fresh one starts at zero)."""
    N = frames.shape[0]
    if frames.dim() != 2 or frames.shape[1] != 9 * int(J):
        raise ValueError(f"rotmat_to_euler: frames must be (N, {9 * int(J)}), got {tuple(frames.shape)}")
    if out is None:
        out = torch.empty((N, 3 * int(J)), dtype=torch.float32, device=frames.device)
    if bad is None:
        bad = torch.zeros((1,), dtype=torch.int64, device=frames.device)
    check(_lib_().g2v_rotmat_to_euler(_p(_chk(frames, name="frames")), _p(_chk(out, name="out")), _p(_chk(bad, torch.int64, "bad")), N,
                                      int(J), int(method), _stream()), "rotmat_to_euler")
    return out, bad


def smoothing_spline(y, smooth, out=None, ws=None):
    """out (B, F, Cn) = the cubic smoothing spline of y (B, F, Cn) along F at the knots (g2v_smoothing_spline): csaps' `smooth` in
    [0, 1].  out may be y itself.  ws: a uint8 workspace of at least g2v_smoothing_spline_workspace(B, F, Cn) bytes (default: the
    reusable one)."""
    if y.dim() != 3:
        raise ValueError(f"smoothing_spline: y must be (B, F, Cn), got {tuple(y.shape)}")
    B, F, Cn = y.shape
    lib = _lib_()
    if out is None:
        out = torch.empty_like(y)
    if ws is None:
        ws = workspace(lib.g2v_smoothing_spline_workspace(B, F, Cn), y.device, "spline")
    check(lib.g2v_smoothing_spline(_p(_chk(y, name="y")), _p(_chk(out, name="out")), float(smooth), B, F, Cn, _p(ws), ws.numel(),
                                   _stream()), "smoothing_spline")
    return out


# ------------------------------------------------------------------------------------------ k-means (kmeans.hip)
KMEANS_STATE = ("done", "n_iter", "n_changed", "shift", "inertia", "n_relocated", "active", "tol_abs")   # the float64[8] state block


def kmeans_update(x, labels, centers, prev_labels=None, *, relocate=True, state=None, out=None):
    """One Lloyd update (g2v_kmeans_update): x (N,E) fp32, labels (N) int64, centers (K,E) -> dict(counts (K) int64, sums (K,E) f64,
    centers_new (K,E) fp32, stats (4) f64 = [inertia vs `centers`, shift, n_changed, n_relocated], relocated_rows (K) int64).
    `out`: the dict of an earlier call, written again.  `state`: the (8,) float64 device block (KMEANS_STATE) that gates the call."""
    N, E = x.shape
    K = centers.shape[0]
    dev = x.device
    if out is None:
        out = {"counts": torch.empty((K,), dtype=torch.int64, device=dev), "sums": torch.empty((K, E), dtype=torch.float64, device=dev),
               "centers_new": torch.empty((K, E), dtype=torch.float32, device=dev),
               "stats": torch.zeros((4,), dtype=torch.float64, device=dev),
               "relocated_rows": torch.full((K,), -1, dtype=torch.int64, device=dev)}
    for key, shape, dtype in (("counts", (K,), torch.int64), ("sums", (K, E), torch.float64), ("centers_new", (K, E), torch.float32),
                              ("stats", (4,), torch.float64), ("relocated_rows", (K,), torch.int64)):
        if tuple(_chk(out[key], dtype, key).shape) != shape:
            raise ValueError(f"kmeans_update: out[{key!r}] must have shape {shape}, got {tuple(out[key].shape)}")
    if labels.numel() != N or (prev_labels is not None and prev_labels.numel() != N) or centers.shape[1] != E:
        raise ValueError("kmeans_update: labels / prev_labels must hold N ids and centers must be (K, E)")
    lib = _lib_()
    nb = int(lib.g2v_kmeans_update_workspace(N, E, K))
    ws = workspace(nb, dev, "kmeans")
    check(lib.g2v_kmeans_update(_p(_chk(x, name="x")), _p(_chk(labels, torch.int64, "labels")),
                                _p(None if prev_labels is None else _chk(prev_labels, torch.int64, "prev_labels")),
                                _p(_chk(centers, name="centers")), N, E, K, 1 if relocate else 0, _p(out["counts"]), _p(out["sums"]),
                                _p(out["centers_new"]), _p(out["stats"]), _p(out["relocated_rows"]),
                                _p(None if state is None else _chk(state, torch.float64, "state")), _p(ws), nb, _stream()),
          "kmeans_update")
    return out


def kmeans_commit(state, centers_new, centers, labels_new=None, labels=None):
    """centers <- centers_new, labels <- labels_new when the last g2v_kmeans_update on `state` ran (g2v_kmeans_commit)."""
    if centers_new.shape != centers.shape or (labels is None) != (labels_new is None):
        raise ValueError("kmeans_commit: centers_new / centers must match in shape, labels_new / labels come together")
    if labels is not None:
        _chk(labels_new, torch.int64, "labels_new")
        _chk(labels, torch.int64, "labels")
        if labels_new.numel() != labels.numel():
            raise ValueError("kmeans_commit: labels_new and labels differ in length")
    check(_lib_().g2v_kmeans_commit(_p(_chk(state, torch.float64, "state")), _p(_chk(centers_new, name="centers_new")),
                                    _p(_chk(centers, name="centers")), centers.numel(), _p(labels_new), _p(labels),
                                    0 if labels is None else labels.numel(), _stream()), "kmeans_commit")


def kmeans_tolerance(x, tol, out=None):
    """(1,) float64 = tol * mean_e Var(x_e) (g2v_kmeans_tolerance; sklearn's _tolerance)."""
    N, E = x.shape
    if out is None:
        out = torch.empty((1,), dtype=torch.float64, device=x.device)
    lib = _lib_()
    nb = int(lib.g2v_kmeans_tolerance_workspace(N, E))
    ws = workspace(nb, x.device, "kmeans_tol")
    check(lib.g2v_kmeans_tolerance(_p(_chk(x, name="x")), N, E, float(tol), _p(out), _p(ws), nb, _stream()), "kmeans_tolerance")
    return out


def kmeans_pp_blocks(N) -> int:
    return int(_lib_().g2v_kmeans_pp_blocks(int(N)))


def kmeans_pp_step(x, closest, pick_block, pick_resid, out, center_out):
    """One greedy k-means++ step (g2v_kmeans_pp_step).  pick_block / pick_resid: host sequences (pick_resid None: pick_block holds the
    candidate rows themselves); out (blocks + 11,) float64; center_out (E,) fp32."""
    N, E = x.shape
    n = len(pick_block)
    blk = (C.c_int64 * n)(*[int(b) for b in pick_block])
    res = None if pick_resid is None else (C.c_double * n)(*[float(r) for r in pick_resid])
    lib = _lib_()
    nb = int(lib.g2v_kmeans_pp_workspace(N, E))
    ws = workspace(nb, x.device, "kmeans_pp")
    check(lib.g2v_kmeans_pp_step(_p(_chk(x, name="x")), N, E, _p(_chk(closest, torch.float64, "closest")), blk, res, n,
                                 _p(_chk(out, torch.float64, "out")), _p(_chk(center_out)), _p(ws), nb, _stream()), "kmeans_pp_step")
    return out


# ------------------------------------------------------------------------------------------ silhouette (silhouette.hip)
def silhouette_samples(x, labels, K):
    """Silhouette terms of the clustering `labels` (N) int64 of the rows of x (N,E) fp32, unit column stride, any row stride that is a
    multiple of 4 (g2v_silhouette_samples) -> dict(a, b, s (N) f64, counts (K+1) int64 with the out-of-range labels in counts[K],
    out (2) f64 = [sum of s, number of non-empty clusters]).  All device tensors; nothing is read back."""
    if not x.is_cuda:
        raise _lib.G2VLibraryError("x must be a GPU tensor: the g2v kernels have no CPU path")
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("silhouette_samples: x must be a (N, E) fp32 tensor with unit column stride")
    N, E = x.shape
    K = int(K)
    if labels.numel() != N:
        raise ValueError("silhouette_samples: labels must hold N ids")
    dev = x.device
    res = {"a": torch.empty((N,), dtype=torch.float64, device=dev), "b": torch.empty((N,), dtype=torch.float64, device=dev),
           "s": torch.empty((N,), dtype=torch.float64, device=dev), "counts": torch.empty((K + 1,), dtype=torch.int64, device=dev),
           "out": torch.empty((2,), dtype=torch.float64, device=dev)}
    lib = _lib_()
    nb = int(lib.g2v_silhouette_workspace(N, E, K))
    ws = workspace(max(nb, 16), dev, "silhouette")
    check(lib.g2v_silhouette_samples(_p(x), int(x.stride(0)), _p(_chk(labels, torch.int64, "labels")), N, E, K, _p(res["a"]),
                                     _p(res["b"]), _p(res["s"]), _p(res["counts"]), _p(res["out"]), _p(ws), nb, _stream()),
          "silhouette_samples")
    return res


# ------------------------------------------------------------------------------------------ DBSCAN (dbscan.hip)
def dbscan_max_rows() -> int:
    return int(_lib_().g2v_dbscan_max_rows())


def dbscan_workspace(N, E) -> int:
    """bytes of workspace of dbscan_neighbors / dbscan_labels; 0 for a shape they refuse"""
    return int(_lib_().g2v_dbscan_workspace(int(N), int(E)))


def dbscan_neighbors(x, eps):
    """-> (bitmap (N, ceil(N / 64)) int64, counts (N) int64) of the rows of x (N, E) fp32, unit column stride, row stride a multiple
    of 4 (g2v_dbscan_neighbors): bit (j % 64) of word j // 64 of row i is set iff |x_i - x_j| <= eps, decided in float64; counts
    is the popcount of each row.  The words are 64 bits each; int64 is the carrier."""
    if not x.is_cuda:
        raise _lib.G2VLibraryError("x must be a GPU tensor: the g2v kernels have no CPU path")
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("dbscan_neighbors: x must be a (N, E) fp32 tensor with unit column stride")
    N, E = x.shape
    if N > dbscan_max_rows():
        raise ValueError(f"dbscan_neighbors: N = {N} exceeds {dbscan_max_rows()} rows (the adjacency bitmap is N^2 / 8 bytes)")
    lib = _lib_()
    nb = dbscan_workspace(N, E)
    ws = workspace(max(nb, 16), x.device, "dbscan")
    bitmap = torch.empty((N, (N + 63) // 64), dtype=torch.int64, device=x.device)
    counts = torch.empty((N,), dtype=torch.int64, device=x.device)
    check(lib.g2v_dbscan_neighbors(_p(x), int(x.stride(0)), N, E, float(eps), _p(bitmap), _p(counts), _p(ws), nb, _stream()),
          "dbscan_neighbors")
    return bitmap, counts


def dbscan_propagate(bitmap, counts, min_samples, L, tmp, *, init, rounds=1):
    """`rounds` rounds of min-propagation with pointer jumping over the core rows, in place on L (N) int32 (tmp: as L)
    (g2v_dbscan_propagate) -> flags (rounds) int32 on the device, flags[r] = 1 iff round r changed a row.  init=True starts L."""
    N = bitmap.shape[0]
    flags = torch.empty((int(rounds),), dtype=torch.int32, device=bitmap.device)
    check(_lib_().g2v_dbscan_propagate(_p(_chk(bitmap, torch.int64, "bitmap")), _p(_chk(counts, torch.int64, "counts")), N,
                                       int(min_samples), 1 if init else 0, int(rounds), _p(_chk(L, torch.int32, "L")),
                                       _p(_chk(tmp, torch.int32, "tmp")), _p(flags), _stream()), "dbscan_propagate")
    return flags


def dbscan_labels(bitmap, L):
    """The converged L -> (labels (N) int64, core (N) uint8, out (3) int64 = [clusters, core rows, noise rows]) (g2v_dbscan_labels)"""
    N = bitmap.shape[0]
    dev = bitmap.device
    labels = torch.empty((N,), dtype=torch.int64, device=dev)
    core = torch.empty((N,), dtype=torch.uint8, device=dev)
    out = torch.empty((3,), dtype=torch.int64, device=dev)
    nb = dbscan_workspace(N, 1)
    ws = workspace(max(nb, 16), dev, "dbscan")
    check(_lib_().g2v_dbscan_labels(_p(_chk(bitmap, torch.int64, "bitmap")), _p(_chk(L, torch.int32, "L")), N, _p(labels), _p(core),
                                    _p(out), _p(ws), nb, _stream()), "dbscan_labels")
    return labels, core, out


# ------------------------------------------------------------------------------------------ Ward linkage (ward.hip)
def ward_max_rows() -> int:
    return int(_lib_().g2v_ward_max_rows())


def ward_workspace(N, E) -> int:
    """bytes of workspace of ward_distances; 0 for a shape it refuses"""
    return int(_lib_().g2v_ward_workspace(int(N), int(E)))


def ward_distances(x):
    """-> D (N, N) float64: the Euclidean (unsquared) distances between the rows of x (N, E) fp32, unit column stride, row stride a
    multiple of 4 (g2v_ward_distances: the rows widened to float64, Gram tiles on the float64 MFMA, near pairs from differences);
    +inf on the diagonal, bitwise symmetric."""
    if not x.is_cuda:
        raise _lib.G2VLibraryError("x must be a GPU tensor: the g2v kernels have no CPU path")
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("ward_distances: x must be a (N, E) fp32 tensor with unit column stride")
    N, E = x.shape
    if N > ward_max_rows():
        raise ValueError(f"ward_distances: N = {N} exceeds {ward_max_rows()} rows (the distance matrix is 8 N^2 bytes)")
    lib = _lib_()
    nb = ward_workspace(N, E)
    ws = workspace(max(nb, 16), x.device, "ward")
    D = torch.empty((N, N), dtype=torch.float64, device=x.device)
    check(lib.g2v_ward_distances(_p(x), int(x.stride(0)), N, E, _p(D), _p(ws), nb, _stream()), "ward_distances")
    return D


def ward_state(N, device):
    """The tensors g2v_ward_rounds keeps between calls: size, nn, part int32 (N); pairs int32 (N - 1, 2), heights float64 (N - 1),
    sizes int32 (N - 1): the merge log; counters int64 (4) = [merges logged, rounds that merged, the last round's merges, its base]"""
    i32 = dict(dtype=torch.int32, device=device)
    return {"size": torch.empty((N,), **i32), "nn": torch.empty((N,), **i32), "part": torch.empty((N,), **i32),
            "pairs": torch.empty((max(N - 1, 1), 2), **i32), "heights": torch.empty((max(N - 1, 1),), dtype=torch.float64, device=device),
            "sizes": torch.empty((max(N - 1, 1),), **i32), "counters": torch.empty((4,), dtype=torch.int64, device=device)}


def ward_rounds(D, state, *, init, rounds=1):
    """`rounds` rounds of mutual-nearest-neighbour merges over D (N, N) float64 from ward_distances, in place, logged into `state`
    (ward_state) (g2v_ward_rounds) -> state["counters"] on the device.  init=True starts the state."""
    N = D.shape[0]
    if tuple(D.shape) != (N, N):
        raise ValueError(f"ward_rounds: D must be square, got {tuple(D.shape)}")
    s = state
    for name in ("size", "nn", "part"):
        if tuple(_chk(s[name], torch.int32, name).shape) != (N,):
            raise ValueError(f"ward_rounds: {name} must be ({N},), got {tuple(s[name].shape)}")
    if s["pairs"].shape[0] < N - 1 or s["heights"].shape[0] < N - 1 or s["sizes"].shape[0] < N - 1:
        raise ValueError("ward_rounds: the merge log holds fewer than N - 1 entries")
    check(_lib_().g2v_ward_rounds(_p(_chk(D, torch.float64, "D")), N, _p(s["size"]), _p(s["nn"]), _p(s["part"]), 1 if init else 0,
                                  int(rounds), _p(_chk(s["pairs"], torch.int32, "pairs")), _p(_chk(s["heights"], torch.float64, "heights")),
                                  _p(_chk(s["sizes"], torch.int32, "sizes")), _p(_chk(s["counters"], torch.int64, "counters")),
                                  _stream()), "ward_rounds")
    return s["counters"]


# ------------------------------------------------------------------------------------------ pairwise-distance statistics (pair_stats.hip)
def pair_stats_max_rows() -> int:
    return int(_lib_().g2v_pair_stats_max_rows())


def pair_stats_max_bins() -> int:
    return int(_lib_().g2v_pair_stats_max_bins())


def pair_stats_run(N, M=0) -> int:
    """64-row tiles of the second set (of x itself with M == 0) that one workgroup of pair_stats takes: a function of the row counts
    alone; 0 for a shape it refuses"""
    return int(_lib_().g2v_pair_stats_run(int(N), int(M)))


def pair_stats_workspace(N, M, E, bins=0) -> int:
    """bytes of workspace of pair_stats; 0 for a shape it refuses"""
    return int(_lib_().g2v_pair_stats_workspace(int(N), int(M), int(E), int(bins)))


def _pair_rows(t, name, what):
    if not t.is_cuda:
        raise _lib.G2VLibraryError(f"{name} must be a GPU tensor: the g2v kernels have no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1:
        raise TypeError(f"{what}: {name} must be a (N, E) fp32 tensor with unit column stride")


def pair_stats(x, y=None, edges=None, *, ws=None):
    """-> (out (4) float64 = [sum d, sum d^2, min d, max d], counts (2) int64 = [pairs, pairs not finite], hist (bins) int64 or None)
    over the Euclidean distances between the rows of x (N, E) fp32, unit column stride, row stride a multiple of 4: the pairs i < j
    of x, or with y (M, E) all N M pairs (g2v_pair_stats: Gram tiles on the float64 MFMA, near pairs from differences, no distance
    stored).  edges: (bins + 1) float64 on the device, ascending (not checked here), counted by numpy.histogram's rule.  ws: a byte
    buffer of at least pair_stats_workspace bytes to use instead of the cached one.  Nothing is read back."""
    _pair_rows(x, "x", "pair_stats")
    N, E = x.shape
    M = 0
    if y is not None:
        _pair_rows(y, "y", "pair_stats")
        M = y.shape[0]
        if y.shape[1] != E or y.device != x.device:
            raise ValueError(f"pair_stats: y must be (M, {E}) on the device of x, got {tuple(y.shape)} on {y.device}")
        if M < 1:
            raise ValueError("pair_stats: y has no rows")
    bins = 0
    if edges is not None:
        bins = _chk(edges, torch.float64, "edges").numel() - 1
        if edges.dim() != 1 or bins < 1:
            raise ValueError(f"pair_stats: edges must be 1-D with at least 2 entries, got {tuple(edges.shape)}")
    lib = _lib_()
    nb = pair_stats_workspace(N, M, E, bins)
    if nb == 0:
        raise ValueError(f"pair_stats: unsupported shape N = {N}, M = {M}, E = {E}, bins = {bins} (1 <= N, M <= {pair_stats_max_rows()}, "
                         f"1 <= E <= 512, bins <= {pair_stats_max_bins()})")
    if ws is None:
        ws = workspace(max(nb, 16), x.device, "pair_stats")
    elif not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < nb:
        raise ValueError(f"pair_stats: ws must be a contiguous uint8 GPU tensor of at least {nb} bytes")
    out = torch.empty((4,), dtype=torch.float64, device=x.device)
    counts = torch.empty((2,), dtype=torch.int64, device=x.device)
    hist = torch.empty((bins,), dtype=torch.int64, device=x.device) if bins else None
    check(lib.g2v_pair_stats(_p(x), int(x.stride(0)), N, _p(y), int(y.stride(0)) if y is not None else 0, M, E, _p(edges), bins, _p(out),
                             _p(counts), _p(hist), _p(ws), nb, _stream()), "pair_stats")
    return out, counts, hist


def lag_distances(x, lags, clip_ids=None):
    """-> (n_lags, N) float64: out[l][i] = (|x_{i - lag} - x_i| + |x_{i + lag} - x_i|) / 2 over the rows of x (N, E) fp32, unit column
    stride, row stride a multiple of 4 (g2v_lag_distances); NaN where a neighbour is past either end or, with clip_ids (N) int64,
    carries another id than row i.  lags: up to 8 host integers >= 1."""
    _pair_rows(x, "x", "lag_distances")
    N, E = x.shape
    lags = [int(v) for v in lags]
    if not 1 <= len(lags) <= 8 or min(lags) < 1 or max(lags) >= 2 ** 31:
        raise ValueError(f"lag_distances: needs 1 to 8 lags, each >= 1, got {lags}")
    if clip_ids is not None and tuple(_chk(clip_ids, torch.int64, "clip_ids").shape) != (N,):
        raise ValueError(f"lag_distances: clip_ids must be ({N},), got {tuple(clip_ids.shape)}")
    out = torch.empty((len(lags), N), dtype=torch.float64, device=x.device)
    arr = (C.c_int32 * len(lags))(*lags)
    check(_lib_().g2v_lag_distances(_p(x), int(x.stride(0)), N, E, arr, len(lags), _p(clip_ids), _p(out), _stream()), "lag_distances")
    return out


# ------------------------------------------------------------------------------------------ DTW k-means (dtw.hip)
def dtw_max_len() -> int:
    return int(_lib_().g2v_dtw_max_len())


def dtw_workspace(N, M, T, S, F) -> int:
    """bytes of workspace of dtw_cdist / dtw_dba_accumulate against M centres; 0 for a shape they refuse"""
    return int(_lib_().g2v_dtw_workspace(int(N), int(M), int(T), int(S), int(F)))


def _dtw_operands(x, y, fn):
    if not x.is_cuda or not y.is_cuda:
        raise _lib.G2VLibraryError(f"{fn}: the series and the centres must be GPU tensors: the g2v kernels have no CPU path")
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError(f"{fn}: the series must be a contiguous (N, T, F) fp32 tensor")
    if y.dim() != 3 or y.dtype != torch.float64 or not y.is_contiguous():
        raise TypeError(f"{fn}: the centres must be a contiguous (M, S, F) float64 tensor")
    if y.shape[2] != x.shape[2]:
        raise ValueError(f"{fn}: the series have {x.shape[2]} columns and the centres {y.shape[2]}")
    if x.shape[0] < 1 or y.shape[0] < 1:
        raise ValueError(f"{fn}: needs at least one series and one centre")
    return x.shape[0], x.shape[1], y.shape[0], y.shape[1], x.shape[2]


def _dtw_ws(N, M, T, S, F, device):
    nb = dtw_workspace(N, M, T, S, F)
    return workspace(max(nb, 16), device, "dtw"), nb


def dtw_cdist(x, y, *, squared=False, want_out=True, want_labels=False):
    """x (N, T, F) fp32 series, y (M, S, F) float64 centres -> (out, labels, best) (g2v_dtw_cdist): out (N, M) float64 = dtw^2 with
    squared=True, else its square root (None without want_out); labels (N) int64 = the argmin over the centres, lowest index on
    ties, best (N) float64 = the minimal dtw^2 (None without want_labels)."""
    N, T, M, S, F = _dtw_operands(x, y, "dtw_cdist")
    if not (want_out or want_labels):
        raise ValueError("dtw_cdist: nothing asked for")
    dev = x.device
    out = torch.empty((N, M), dtype=torch.float64, device=dev) if want_out else None
    labels = torch.empty((N,), dtype=torch.int64, device=dev) if want_labels else None
    best = torch.empty((N,), dtype=torch.float64, device=dev) if want_labels else None
    ws, nb = _dtw_ws(N, M, T, S, F, dev)
    check(_lib_().g2v_dtw_cdist(_p(x), N, T, _p(y), M, S, F, 1 if squared else 0, _p(out), _p(labels), _p(best), _p(ws), nb, _stream()),
          "dtw_cdist")
    return out, labels, best


def dtw_dba_state(K, device):
    """The stop-rule block of g2v_dtw_dba_update as one byte tensor -> (state, prev_cost (K) float64 view, live (K) uint8 view),
    started at +inf and 1"""
    state = torch.empty((9 * int(K),), dtype=torch.uint8, device=device)
    prev, live = state[:8 * K].view(torch.float64), state[8 * K:]
    prev.fill_(float("inf"))
    live.fill_(1)
    return state, prev, live


def dtw_dba_accumulate(x, labels, centers, live=None, out=None):
    """One DBA assignment pass (g2v_dtw_dba_accumulate): per live cluster k, over the warping paths of its rows against centers[k]
    -> dict sums (K, S, F) float64, counts (K, S) int64, cost (K) float64; `out`: such a dict to write into (clusters that are not
    live keep what it holds).  labels (N) int64; live (K) uint8 or None."""
    N, T, K, S, F = _dtw_operands(x, centers, "dtw_dba_accumulate")
    dev = x.device
    if tuple(_chk(labels, torch.int64, "labels").shape) != (N,):
        raise ValueError(f"dtw_dba_accumulate: labels must be ({N},), got {tuple(labels.shape)}")
    if live is not None and tuple(_chk(live, torch.uint8, "live").shape) != (K,):
        raise ValueError(f"dtw_dba_accumulate: live must be ({K},), got {tuple(live.shape)}")
    if out is None:
        out = {"sums": torch.zeros((K, S, F), dtype=torch.float64, device=dev),
               "counts": torch.zeros((K, S), dtype=torch.int64, device=dev), "cost": torch.zeros((K,), dtype=torch.float64, device=dev)}
    if tuple(_chk(out["sums"], torch.float64, "sums").shape) != (K, S, F) or \
            tuple(_chk(out["counts"], torch.int64, "counts").shape) != (K, S) or \
            tuple(_chk(out["cost"], torch.float64, "cost").shape) != (K,):
        raise ValueError("dtw_dba_accumulate: out must hold sums (K, S, F), counts (K, S) and cost (K)")
    ws, nb = _dtw_ws(N, K, T, S, F, dev)
    check(_lib_().g2v_dtw_dba_accumulate(_p(x), N, T, _p(labels), _p(centers), K, S, F, _p(live), _p(out["sums"]), _p(out["counts"]),
                                         _p(out["cost"]), _p(ws), nb, _stream()), "dtw_dba_accumulate")
    return out


def dtw_dba_update(acc, members, state, centers, tol):
    """One barycentre step per live cluster, in place on centers (K, S, F) float64 and on state (dtw_dba_state)
    (g2v_dtw_dba_update); acc: the dict of dtw_dba_accumulate, members (K) int64: the rows of each cluster."""
    K, S, F = _chk(centers, torch.float64, "centers").shape
    if state.dtype != torch.uint8 or state.numel() != 9 * K or not state.is_contiguous():
        raise ValueError(f"dtw_dba_update: state must be the {9 * K} bytes of dtw_dba_state")
    if tuple(_chk(members, torch.int64, "members").shape) != (K,):
        raise ValueError(f"dtw_dba_update: members must be ({K},), got {tuple(members.shape)}")
    check(_lib_().g2v_dtw_dba_update(_p(_chk(acc["sums"], torch.float64, "sums")), _p(_chk(acc["counts"], torch.int64, "counts")),
                                     _p(_chk(acc["cost"], torch.float64, "cost")), _p(members), _p(_chk(state, torch.uint8, "state")),
                                     _p(centers), K, S, F, float(tol), _stream()), "dtw_dba_update")
    return centers


# ------------------------------------------------------------------------------------------ soft-DTW (softdtw.hip)
def softdtw_workspace(N, M, T, S, F) -> int:
    """bytes of workspace of softdtw_cdist over N series and M centres, or of softdtw_grad over N member rows (M = 1); 0 for a shape
    they refuse"""
    return int(_lib_().g2v_softdtw_workspace(int(N), int(M), int(T), int(S), int(F)))


def _softdtw_ws(N, M, T, S, F, device):
    nb = softdtw_workspace(N, M, T, S, F)
    return workspace(max(nb, 16), device, "softdtw"), nb


def softdtw_cdist(x, y, gamma, *, want_out=True, want_labels=False):
    """x (N, T, F) fp32 series, y (M, S, F) float64 centres -> (out, labels, best) (g2v_softdtw_cdist): out (N, M) float64 =
    sdtw_gamma(y_m, x_n) (None without want_out); labels (N) int64 = the argmin over the centres, lowest index on ties, best (N)
    float64 = the minimal value (None without want_labels)."""
    N, T, M, S, F = _dtw_operands(x, y, "softdtw_cdist")
    if not (want_out or want_labels):
        raise ValueError("softdtw_cdist: nothing asked for")
    dev = x.device
    out = torch.empty((N, M), dtype=torch.float64, device=dev) if want_out else None
    labels = torch.empty((N,), dtype=torch.int64, device=dev) if want_labels else None
    best = torch.empty((N,), dtype=torch.float64, device=dev) if want_labels else None
    ws, nb = _softdtw_ws(N, M, T, S, F, dev)
    check(_lib_().g2v_softdtw_cdist(_p(x), N, T, _p(y), M, S, F, float(gamma), _p(out), _p(labels), _p(best), _p(ws), nb, _stream()),
          "softdtw_cdist")
    return out, labels, best


def softdtw_alignment(x, z, gamma):
    """x (R, T, F) fp32 rows, z (S, F) float64: one centre -> (E (R, S, T) float64: the soft alignment matrix of every row, value (R)
    float64 = sdtw_gamma(z, x_r)) (g2v_softdtw_alignment)"""
    R, T, _, S, F = _dtw_operands(x, z[None] if z.dim() == 2 else z, "softdtw_alignment")
    if z.dim() != 2:
        raise TypeError("softdtw_alignment: the centre must be a (S, F) float64 tensor")
    E = torch.empty((R, S, T), dtype=torch.float64, device=x.device)
    value = torch.empty((R,), dtype=torch.float64, device=x.device)
    check(_lib_().g2v_softdtw_alignment(_p(x), R, T, _p(z), S, F, float(gamma), _p(value), _p(E), _stream()), "softdtw_alignment")
    return E, value


def softdtw_grad(x, rows, z, gamma, weights=None, out=None):
    """One evaluation of a barycentre objective (g2v_softdtw_grad): x (N, T, F) fp32, rows (R) int64 on the device, ascending member
    row ids, z (S, F) float64, weights (R) float64 or None (all ones) -> (value (1), grad (S, F)): views of one float64 tensor of
    1 + S F elements, `out` when given, so that both reach the host in one copy."""
    N, T, _, S, F = _dtw_operands(x, z[None] if z.dim() == 2 else z, "softdtw_grad")
    if z.dim() != 2:
        raise TypeError("softdtw_grad: the centre must be a (S, F) float64 tensor")
    R = _chk(rows, torch.int64, "rows").numel()
    if rows.dim() != 1 or R < 1:
        raise ValueError(f"softdtw_grad: rows must be a non-empty 1-D tensor, got {tuple(rows.shape)}")
    if weights is not None and tuple(_chk(weights, torch.float64, "weights").shape) != (R,):
        raise ValueError(f"softdtw_grad: weights must be ({R},), got {tuple(weights.shape)}")
    if out is None:
        out = torch.empty((1 + S * F,), dtype=torch.float64, device=x.device)
    if tuple(_chk(out, torch.float64, "out").shape) != (1 + S * F,):
        raise ValueError(f"softdtw_grad: out must be ({1 + S * F},) float64")
    value, grad = out[:1], out[1:].view(S, F)
    ws, nb = _softdtw_ws(R, 1, T, S, F, x.device)
    check(_lib_().g2v_softdtw_grad(_p(x), N, T, _p(rows), R, _p(weights), _p(z), S, F, float(gamma), _p(value), _p(grad), _p(ws), nb,
                                   _stream()), "softdtw_grad")
    return value, grad


# ------------------------------------------------------------------------------------------ exact t-SNE (tsne.hip)
def tsne_max_rows() -> int:
    return int(_lib_().g2v_tsne_max_rows())


def tsne_affinities(x, perplexity):
    """The joint P (N, N) fp32 of exact t-SNE over the rows of x (N, d) fp32, unit column stride, row stride a multiple of 4
    (g2v_tsne_affinities: Gram distances, sklearn's per-row bisection of the precision, symmetrised; symmetric, diagonal 0)."""
    if not x.is_cuda:
        raise _lib.G2VLibraryError("x must be a GPU tensor: the g2v kernels have no CPU path")
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("tsne_affinities: x must be a (N, d) fp32 tensor with unit column stride")
    N, d = x.shape
    if not 2 <= N <= tsne_max_rows():
        raise ValueError(f"tsne_affinities: N = {N} outside [2, {tsne_max_rows()}]")
    lib = _lib_()
    nb = int(lib.g2v_tsne_affinities_workspace(N, d))
    ws = workspace(max(nb, 16), x.device, "tsne")
    out = torch.empty((N, N), dtype=torch.float32, device=x.device)
    check(lib.g2v_tsne_affinities(_p(x), int(x.stride(0)), N, d, float(perplexity), _p(out), _p(ws), nb, _stream()), "tsne_affinities")
    return out


def tsne_gradient(P, y, exaggeration=1.0, want_kl=True, *, grad=None, out=None):
    """-> (grad (N, 2) fp32, out (3,) float64 = [KL, sum grad^2, Z]) of the t-SNE objective at y (N, 2) fp32 for the joint P
    (g2v_tsne_gradient: one pass over P, float64 sums in a fixed order; KL is NaN with want_kl=False)."""
    N = y.shape[0]
    if tuple(y.shape) != (N, 2) or tuple(P.shape) != (N, N):
        raise ValueError(f"tsne_gradient: y must be (N, 2) and P (N, N), got {tuple(y.shape)} and {tuple(P.shape)}")
    if grad is None:
        grad = torch.empty((N, 2), dtype=torch.float32, device=y.device)
    if out is None:
        out = torch.empty((3,), dtype=torch.float64, device=y.device)
    lib = _lib_()
    nb = int(lib.g2v_tsne_gradient_workspace(N))
    ws = workspace(max(nb, 16), y.device, "tsne_grad")
    check(lib.g2v_tsne_gradient(_p(_chk(P, name="P")), _p(_chk(y, name="y")), N, float(exaggeration), 1 if want_kl else 0,
                                _p(_chk(grad, name="grad")), _p(_chk(out, torch.float64, "out")), _p(ws), nb, _stream()), "tsne_gradient")
    return grad, out


def tsne_update(y, velocity, gains, grad, momentum, learning_rate, gnorm2=None):
    """One step of sklearn's _gradient_descent over y, velocity, gains (N, 2) fp32, in place (g2v_tsne_update); gnorm2: (1,) float64
    that receives sum (gains grad)^2."""
    N = y.shape[0]
    for name, t in (("y", y), ("velocity", velocity), ("gains", gains), ("grad", grad)):
        if tuple(_chk(t, name=name).shape) != (N, 2):
            raise ValueError(f"tsne_update: {name} must be ({N}, 2), got {tuple(t.shape)}")
    check(_lib_().g2v_tsne_update(_p(y), _p(velocity), _p(gains), _p(grad), N, float(momentum), float(learning_rate),
                                  _p(None if gnorm2 is None else _chk(gnorm2, torch.float64, "gnorm2")), _stream()), "tsne_update")
    return y


# ------------------------------------------------------------------- new rows into a fitted t-SNE map (tsne_place.hip)
def _place_rows(t, name, fn):
    if not t.is_cuda:
        raise _lib.G2VLibraryError(f"{name} must be a GPU tensor: the g2v kernels have no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.data_ptr() % 16 != 0:
        raise TypeError(f"{fn}: {name} must be a 16-byte aligned (rows, d) fp32 tensor with unit column stride and a row stride "
                        "that is a multiple of 4")
    return t


def tsne_place_neighbors(x, z, kk):
    """-> (idx (M, kk) int32, d2 (M, kk) fp32): per row of z (M, d) its kk nearest rows of x (N, d) in ascending (d^2, index)
    order, the squared distances formed as tsne_affinities forms them (g2v_tsne_place_neighbors; the M x N distances are never
    stored)."""
    fn = "tsne_place_neighbors"
    x, z = _place_rows(x, "x", fn), _place_rows(z, "z", fn)
    (N, d), M, kk = x.shape, z.shape[0], int(kk)
    if z.shape[1] != d:
        raise ValueError(f"{fn}: x has {d} columns and z {z.shape[1]}")
    lib = _lib_()
    nb = int(lib.g2v_tsne_place_neighbors_workspace(N, M, d, kk))
    if nb == 0:
        raise ValueError(f"{fn}: needs 1 <= d <= 512, 1 <= kk <= min(N, 128), N < 2^24 and M >= 1 (N = {N}, M = {M}, d = {d}, "
                         f"kk = {kk})")
    ws = workspace(nb, x.device, "tsne_place")
    idx = torch.empty((M, kk), dtype=torch.int32, device=x.device)
    d2 = torch.empty((M, kk), dtype=torch.float32, device=x.device)
    check(lib.g2v_tsne_place_neighbors(_p(x), int(x.stride(0)), N, _p(z), int(z.stride(0)), M, d, kk, _p(idx), _p(d2), _p(ws), nb,
                                       _stream()), fn)
    return idx, d2


def tsne_place_conditionals(d2, k_aff, perplexity):
    """-> p (M, k_aff) fp32: the conditionals over the first k_aff columns of d2 (M, kk) at this perplexity, each row summing to 1
    (g2v_tsne_place_conditionals: sklearn's bisection of the precision in float64)."""
    M, kk = _chk(d2, name="d2").shape
    p = torch.empty((M, int(k_aff)), dtype=torch.float32, device=d2.device)
    check(_lib_().g2v_tsne_place_conditionals(_p(d2), M, kk, int(k_aff), float(perplexity), _p(p), _stream()),
          "tsne_place_conditionals")
    return p


def tsne_place_init(Y, idx, p=None, mode="median", k_use=None):
    """-> y (M, 2) fp32, the start of the new rows in the map Y (N, 2): "median" of Y over the first k_use columns of idx (M, kk)
    (numpy's rule), or "weighted" = sum_j p_ij Y_j over the first k_use columns of p (M, k_aff) (g2v_tsne_place_init)."""
    if mode not in ("median", "weighted"):
        raise ValueError(f"tsne_place_init: mode must be 'median' or 'weighted' (got {mode!r})")
    M, kk = _chk(idx, torch.int32, "idx").shape
    N = _chk(Y, name="Y").shape[0]
    if tuple(Y.shape) != (N, 2):
        raise ValueError(f"tsne_place_init: Y must be (N, 2), got {tuple(Y.shape)}")
    weighted = mode == "weighted"
    if weighted and (p is None or _chk(p, name="p").shape[0] != M):
        raise ValueError("tsne_place_init: the weighted start needs p (M, k_aff)")
    k_aff = int(p.shape[1]) if p is not None else 0
    k_use = int(k_use) if k_use is not None else (k_aff if weighted else kk)
    y = torch.empty((M, 2), dtype=torch.float32, device=Y.device)
    check(_lib_().g2v_tsne_place_init(_p(Y), N, _p(idx), _p(p), M, kk, k_aff, 1 if weighted else 0, k_use, _p(y), _stream()),
          "tsne_place_init")
    return y


def tsne_place_descent(Y, idx, p, y, velocity=None, gains=None, n_iter=250, exaggeration=1.5, momentum=0.8, learning_rate=0.1,
                       max_grad_norm=0.25, want=("kl", "zsum", "grad")):
    """n_iter placement steps on y (M, 2) in place (velocity, gains too; fresh ones are made when they are None) against the fixed
    map Y (N, 2), all inside one launch (g2v_tsne_place_descent) -> dict of the per-row outputs named in `want`, evaluated at the
    final y at exaggeration 1: kl (M,) float64, zsum (M,) float64, grad (M, 2) fp32 (unclipped).  n_iter == 0 only evaluates them at
    y, the gradient at the exaggeration given."""
    M, kk = _chk(idx, torch.int32, "idx").shape
    N, k_aff = _chk(Y, name="Y").shape[0], _chk(p, name="p").shape[1]
    if tuple(Y.shape) != (N, 2) or tuple(_chk(y, name="y").shape) != (M, 2) or p.shape[0] != M:
        raise ValueError(f"tsne_place_descent: Y must be (N, 2), y (M, 2), idx (M, kk) and p (M, k_aff); got {tuple(Y.shape)}, "
                         f"{tuple(y.shape)}, {tuple(idx.shape)}, {tuple(p.shape)}")
    if int(n_iter) > 0:
        velocity = torch.zeros_like(y) if velocity is None else velocity
        gains = torch.ones_like(y) if gains is None else gains
        for name, t in (("velocity", velocity), ("gains", gains)):
            if tuple(_chk(t, name=name).shape) != (M, 2):
                raise ValueError(f"tsne_place_descent: {name} must be ({M}, 2), got {tuple(t.shape)}")
    else:
        velocity = gains = None
    out = {}
    if "kl" in want:
        out["kl"] = torch.empty((M,), dtype=torch.float64, device=y.device)
    if "zsum" in want:
        out["zsum"] = torch.empty((M,), dtype=torch.float64, device=y.device)
    if "grad" in want:
        out["grad"] = torch.empty((M, 2), dtype=torch.float32, device=y.device)
    check(_lib_().g2v_tsne_place_descent(_p(Y), N, _p(idx), _p(p), M, kk, k_aff, _p(y), _p(velocity), _p(gains), int(n_iter),
                                         float(exaggeration), float(momentum), float(learning_rate), float(max_grad_norm),
                                         _p(out.get("kl")), _p(out.get("zsum")), _p(out.get("grad")), _stream()),
          "tsne_place_descent")
    return out


# ------------------------------------------------------------------- ranks of given neighbours among all rows (map_quality.hip)
def neighbor_ranks(x, z, idx, self_rows=None):
    """-> (rank (M, k) int32, redecided (1,) int64 on the device): rank[m][s] = 1 + the number of rows l of x (N, d), l != self_rows[m],
    with (|z_m - x_l|^2, l) < (|z_m - x_j|^2, j) for j = idx[m][s], distances in float64 from the differences; 0 where j is outside
    [0, N) or equal to self_rows[m] (g2v_neighbor_ranks; the M x N distances are never stored).  z (M, d) are the query rows, idx
    (M, k) int32 rows of x, self_rows (M,) int64 the row of x that is query m (-1 or None: none).  redecided counts the pairs
    whose fp32 distance lay too close to a threshold to decide on and that were evaluated again in float64."""
    fn = "neighbor_ranks"
    x, z = _place_rows(x, "x", fn), _place_rows(z, "z", fn)
    (N, d), M = x.shape, z.shape[0]
    if z.shape[1] != d:
        raise ValueError(f"{fn}: x has {d} columns and z {z.shape[1]}")
    if _chk(idx, torch.int32, "idx").dim() != 2 or idx.shape[0] != M:
        raise ValueError(f"{fn}: idx must be ({M}, k), got {tuple(idx.shape)}")
    k = int(idx.shape[1])
    if self_rows is not None and tuple(_chk(self_rows, torch.int64, "self_rows").shape) != (M,):
        raise ValueError(f"{fn}: self_rows must be ({M},), got {tuple(self_rows.shape)}")
    lib = _lib_()
    nb = int(lib.g2v_neighbor_ranks_workspace(N, M, d, k))
    if nb == 0:
        raise ValueError(f"{fn}: needs 1 <= d <= 512, 1 <= k <= 127, 1 <= N < 2^24 and 1 <= M < 2^31 (N = {N}, M = {M}, d = {d}, "
                         f"k = {k})")
    ws = workspace(nb, x.device, "neighbor_ranks")
    rank = torch.empty((M, k), dtype=torch.int32, device=x.device)
    redecided = torch.empty((1,), dtype=torch.int64, device=x.device)
    check(lib.g2v_neighbor_ranks(_p(x), int(x.stride(0)), N, _p(z), int(z.stride(0)), M, d, _p(self_rows), _p(idx), k, _p(rank),
                                 _p(redecided), _p(ws), nb, _stream()), fn)
    return rank, redecided


# ------------------------------------------------------------------- the frame-level quantised autoencoder of Part a (vq_frame.hip)
def vqframe_plan(B, D, L, K, training):
    """g2v_vqframe_plan in words -> (route, fused_ok, reason): route "fused" / "staged" is what `auto` takes, "" a refused shape;
    fused_ok says whether the fused kernel of that mode admits the shape at all."""
    lib, c = _lib_(), _lib.CONSTANTS
    args = (int(B), int(D), int(L), int(K), int(bool(training)))
    r = int(lib.g2v_vqframe_plan(*args))
    route = {c["G2V_VQFRAME_FUSED"]: "fused", c["G2V_VQFRAME_STAGED"]: "staged"}.get(r & 255, "")
    return route, bool(r & c["G2V_VQFRAME_FUSED_OK"]), lib.g2v_vqframe_plan_reason(*args).decode()


def vqframe_step(x, target, keep, scale, w_enc, b_enc, bn_w, bn_b, running_mean, running_var, momentum, w_dec, b_dec, codebook,
                 ema_w, ema_cs, commitment, decay, epsilon, grads, want_latent=False, want_out=False):
    """g2v_vqframe_step: training forward + backward of one (B,D) batch in one launch.  grads: the six gradient buffers in the
    order (w_enc, b_enc, bn_w, bn_b, w_dec, b_dec) -- slices of an optimiser's flat gradient, say.  Updates the running statistics
    and the quantiser's state in place -> (scalars (3,) = mse, loss_vq, perplexity; ids int64 (B,); latent or None; out or None)."""
    lib = _lib_()
    B, D = x.shape
    L, K = w_enc.shape[0], codebook.shape[0]
    nb = int(lib.g2v_vqframe_workspace(B, D, L, K, 1))
    if nb == 0:
        raise ValueError("vqframe_step: " + lib.g2v_vqframe_plan_reason(B, D, L, K, 1).decode())
    dev = x.device
    ws = workspace(nb, dev, "vqframe_step")
    scalars = torch.empty((3,), dtype=torch.float32, device=dev)
    ids = torch.empty((B,), dtype=torch.int64, device=dev)
    latent = torch.empty((B, L), dtype=torch.float32, device=dev) if want_latent else None
    out = torch.empty((B, D), dtype=torch.float32, device=dev) if want_out else None
    if keep is not None and tuple(_chk(keep, torch.uint8, "keep").shape) != (B, D):
        raise ValueError(f"vqframe_step: keep must be ({B}, {D}), got {tuple(keep.shape)}")
    if tuple(target.shape) != (B, D):
        raise ValueError(f"vqframe_step: target must be ({B}, {D}), got {tuple(target.shape)}")
    for g, ref in zip(grads, (w_enc, b_enc, bn_w, bn_b, w_dec, b_dec)):
        if _chk(g, name="grad").numel() != ref.numel():
            raise ValueError("vqframe_step: a gradient buffer does not match its parameter")
    check(lib.g2v_vqframe_step(_p(_chk(x, name="x")), _p(_chk(target, name="target")), _p(keep), float(scale), _p(_chk(w_enc)),
                               _p(_chk(b_enc)), _p(_chk(bn_w)), _p(_chk(bn_b)), _p(_chk(running_mean)), _p(_chk(running_var)),
                               float(momentum), _p(_chk(w_dec)), _p(_chk(b_dec)), _p(_chk(codebook)), _p(_chk(ema_w)),
                               _p(_chk(ema_cs)), float(commitment), float(decay), float(epsilon), *[_p(g) for g in grads],
                               _p(scalars), _p(ids), _p(latent), _p(out), _p(ws), nb, B, D, L, K, _stream()), "vqframe_step")
    return scalars, ids, latent, out


def vqframe_infer(x, w_enc, b_enc, bn_w, bn_b, running_mean, running_var, codebook, w_dec=None, b_dec=None, want_latent=False,
                  want_out=False):
    """g2v_vqframe_infer: eval-mode code ids of N frames (running statistics, no dropout) -> (ids int64 (N,), latent or None, out or None)"""
    lib = _lib_()
    N, D = x.shape
    L, K = w_enc.shape[0], codebook.shape[0]
    nb = int(lib.g2v_vqframe_workspace(N, D, L, K, 0))
    if nb == 0:
        raise ValueError("vqframe_infer: " + lib.g2v_vqframe_plan_reason(N, D, L, K, 0).decode())
    dev = x.device
    ws = workspace(nb, dev, "vqframe_infer")
    ids = torch.empty((N,), dtype=torch.int64, device=dev)
    latent = torch.empty((N, L), dtype=torch.float32, device=dev) if want_latent else None
    out = torch.empty((N, D), dtype=torch.float32, device=dev) if want_out else None
    check(lib.g2v_vqframe_infer(_p(_chk(x, name="x")), N, _p(_chk(w_enc)), _p(_chk(b_enc)), _p(_chk(bn_w)), _p(_chk(bn_b)),
                                _p(_chk(running_mean)), _p(_chk(running_var)), _p(_chk(codebook)),
                                _p(w_dec) if want_out else None, _p(b_dec) if want_out else None, _p(ids), _p(latent), _p(out),
                                _p(ws), nb, D, L, K, _stream()), "vqframe_infer")
    return ids, latent, out


# ------------------------------------------------------------------- the frame-level variational autoencoder of Part a (vae_frame.hip)
def vaeframe_plan(B, D, L, training):
    """g2v_vaeframe_plan in words -> (route, fused_ok, reason), as vqframe_plan: route "fused" / "staged" is what `auto` takes, ""
    a refused shape; fused_ok says whether the fused step admits the shape at all."""
    lib, c = _lib_(), _lib.CONSTANTS
    args = (int(B), int(D), int(L), int(bool(training)))
    r = int(lib.g2v_vaeframe_plan(*args))
    route = {c["G2V_VQFRAME_FUSED"]: "fused", c["G2V_VQFRAME_STAGED"]: "staged"}.get(r & 255, "")
    return route, bool(r & c["G2V_VQFRAME_FUSED_OK"]), lib.g2v_vaeframe_plan_reason(*args).decode()


def vaeframe_step(x, target, keep, scale, weights, kl_weight, grads, *, eps=None, seed=0, offset_counter=None, want_latent=False,
                  want_stats=False, want_out=False):
    """g2v_vaeframe_step: training forward + backward of one (B,D) batch in one launch.  weights / grads: the ten tensors / gradient
    buffers in the order (w_enc, b_enc, w_mean, b_mean, w_std, b_std, w_fc, b_fc, w_dec, b_dec) -- slices of an optimiser's flat
    gradient, say.  Noise: `eps` (B,L), or drawn from the Philox stream (seed, offset_counter: device int64, advanced by 1).
    -> dict scalars (3,) = mse, kl, mse + kl_weight kl; eps (the noise used); latent, mean, logvar (B,L) and out (B,D) or None."""
    lib = _lib_()
    B, D = x.shape
    L = weights[0].shape[0]
    nb = int(lib.g2v_vaeframe_workspace(B, D, L))
    if nb == 0:
        raise ValueError("vaeframe_step: " + lib.g2v_vaeframe_plan_reason(B, D, L, 1).decode())
    dev = x.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)      # noqa: E731
    ws = workspace(nb, dev, "vaeframe_step")
    if keep is not None and tuple(_chk(keep, torch.uint8, "keep").shape) != (B, D):
        raise ValueError(f"vaeframe_step: keep must be ({B}, {D}), got {tuple(keep.shape)}")
    if tuple(target.shape) != (B, D):
        raise ValueError(f"vaeframe_step: target must be ({B}, {D}), got {tuple(target.shape)}")
    shapes = ((L, D), (L,), (L, L), (L,), (L, L), (L,), (L, L), (L,), (D, L), (D,))
    if len(weights) != 10 or len(grads) != 10:
        raise ValueError("vaeframe_step: ten weights and ten gradient buffers")
    for wt, g, s in zip(weights, grads, shapes):
        if tuple(_chk(wt, name="weight").shape) != s or _chk(g, name="grad").numel() != wt.numel():
            raise ValueError(f"vaeframe_step: expected a weight of shape {s} and a gradient buffer of its size")
    if eps is not None and tuple(_chk(eps, name="eps").shape) != (B, L):
        raise ValueError(f"vaeframe_step: eps must be ({B}, {L}), got {tuple(eps.shape)}")
    if eps is None and offset_counter is None:
        raise ValueError("vaeframe_step: drawing the noise needs offset_counter")
    o = {"scalars": f(3), "eps": f(B, L) if eps is None else eps, "latent": f(B, L) if want_latent else None,
         "mean": f(B, L) if want_stats else None, "logvar": f(B, L) if want_stats else None, "out": f(B, D) if want_out else None}
    check(lib.g2v_vaeframe_step(_p(_chk(x, name="x")), _p(_chk(target, name="target")), _p(keep), float(scale),
                                *[_p(wt) for wt in weights], float(kl_weight), _p(eps), int(seed), _p(offset_counter),
                                *[_p(g) for g in grads], _p(o["scalars"]), _p(o["latent"]), _p(o["mean"]), _p(o["logvar"]), _p(o["out"]),
                                _p(o["eps"]) if eps is None else None, _p(ws), nb, B, D, L, _stream()), "vaeframe_step")
    return o


def tanh_bwd(dy, y):
    """dpre = dy (1 - y^2), y = tanh(pre)"""
    dpre = torch.empty_like(y)
    check(_lib_().g2v_tanh_bwd(_p(_chk(dy, name="dy")), _p(_chk(y, name="y")), _p(dpre), y.numel(), _stream()), "tanh_bwd")
    return dpre


def reparam_fwd(mean, logvar, *, eps=None, seed=0, offset_counter=None, sample=True):
    """z = mean + exp(logvar / 2) eps over any shape, kl (1,) = mean(exp(logvar) - logvar - 1 + mean^2) -> (z, eps used or None, kl).
    Noise as in vae_latent_fwd: `eps`, or drawn from the Philox stream (seed, offset_counter, advanced by 1); sample=False: z = mean."""
    lib = _lib_()
    n = mean.numel()
    draw = bool(sample) and eps is None
    z, kl = torch.empty_like(mean), torch.empty((1,), dtype=torch.float32, device=mean.device)
    used = (torch.empty_like(mean) if draw else eps) if sample else None
    nb = int(lib.g2v_reparam_workspace(n))
    ws = workspace(nb, mean.device, "reparam")
    check(lib.g2v_reparam_fwd(_p(_chk(mean, name="mean")), _p(_chk(logvar, name="logvar")),
                              _p(_chk(eps, name="eps")) if eps is not None else None, int(seed), _p(offset_counter), int(bool(sample)),
                              _p(z), _p(used) if draw else None, _p(kl), _p(ws), nb, n, _stream()), "reparam_fwd")
    return z, used, kl


def reparam_bwd(dz, g_kl, mean, logvar, eps, g_mean=None, g_logvar=None):
    """Backward of reparam_fwd: dz = d loss / d z or None (0), g_kl = device scalar d loss / d kl or None (0), eps None when the forward
    did not sample, g_mean / g_logvar = gradients reaching mean / logvar directly or None -> (dmean, dlogvar)."""
    dmean, dlogvar = torch.empty_like(mean), torch.empty_like(mean)
    opt = lambda t, name: _p(_chk(t, name=name)) if t is not None else None      # noqa: E731
    check(_lib_().g2v_reparam_bwd(opt(dz, "dz"), _p(g_kl), opt(g_mean, "g_mean"), opt(g_logvar, "g_logvar"), _p(_chk(mean, name="mean")),
                                  _p(_chk(logvar, name="logvar")), opt(eps, "eps"), _p(dmean), _p(dlogvar), mean.numel(), _stream()),
          "reparam_bwd")
    return dmean, dlogvar

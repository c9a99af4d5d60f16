"""GPU residency: a Plan's weights and execution contexts on one device.

What kernels a plan runs, on which buffers, is decided without a GPU in
engine/emit.py: a call template per (plan, batch bucket, dtype) whose
pointers are (region key, offset) descriptors. This module gives the
template memory (all ahead of the hot path):
  * weights: one bf16 master blob in the layout emit.blob_layout fixes,
    plus layout transforms keyed as the template names them — GEMM/conv
    weights pre-transposed to [N][K] bf16 with K zero-padded to a
    multiple of 64 so both MFMA fragments read contiguously along K
    (see csrc/ops/gemm.hip), fp8 GEMM weights with row scales — computed
    on first use or restored from the plan's pinned transform arena;
  * per-batch-bucket ExecContexts: a workspace arena, the template's
    region keys resolved to base addresses, the calls rebased by
    ext.instantiate_plan; optionally hipGraph-captured;
  * the per-request path is: H2D feed copies -> ExecPlan.run ->
    D2H fetches. Weights stay resident (the HBM3E model pool).

Torch is used for memory management and H2D/D2H only — all math runs in
the hand-written HIP kernels (the extension fails loudly if missing on a
GPU box; no silent eager fallback).
"""
from __future__ import annotations

import contextlib
import logging
import threading
from typing import Dict, List, Optional, Tuple

import warnings

import numpy as np

from .emit import (WS, _pad64, _pad128, _pad256b, blob_layout,
                   build_template)
from .planner import Plan, is_sym, resolve_dim

# weight arrays from memory-mapped SavedModels are read-only; we only
# ever READ the torch views of them (H2D staging), so the non-writable
# warning is noise
warnings.filterwarnings(
    "ignore", message="The given NumPy array is not writable")

log = logging.getLogger("tfsc.gpu")

_torch = None
_ext = None
_import_lock = threading.Lock()


class GpuUnavailable(RuntimeError):
    pass


class ModelReleasedError(RuntimeError):
    """Raised when a request races a pool eviction; callers re-fetch."""


def _load_backend():
    """Import torch + the HIP extension. Loud failure on GPU boxes."""
    global _torch, _ext
    with _import_lock:
        if _ext is not None:
            return _torch, _ext
        import torch
        if not torch.cuda.is_available():
            raise GpuUnavailable("no ROCm GPU visible")
        try:
            from . import _tfsc_engine as ext
        except ImportError as e:
            raise GpuUnavailable(
                "GPU present but the tfsc HIP engine extension is not "
                "built — run `PYTORCH_ROCM_ARCH=gfx950 python setup.py "
                f"build_ext --inplace` ({e})") from e
        _torch, _ext = torch, ext
        return torch, ext


def gpu_available() -> bool:
    try:
        _load_backend()
        return True
    except Exception:       # noqa: BLE001
        return False


# shared pinned staging for weight uploads (64 MiB bf16), reused across
# model loads under a lock — page-locking memory per load is slower than
# the copies it serves
_staging_lock = threading.Lock()
_staging_buf = None


def _get_staging(torch):
    global _staging_buf
    if _staging_buf is None:
        _staging_buf = torch.empty(32 * 1024 * 1024, dtype=torch.bfloat16,
                                   pin_memory=True)
    return _staging_buf


# ---------------------------------------------------------------------------
# capture/upload coordination.
#
# Round-1 finding (ROADMAP item 8): pinned host allocation (hipHostMalloc)
# and DMAs sourced from freshly-allocated host blobs, issued WHILE another
# thread is inside hipStreamBeginCapture..EndCapture, poison the capture —
# replay then fails with "previous error during capture" — even though
# captures use hipStreamCaptureModeThreadLocal. Loads and captures overlap
# by design under LRU churn, so the two operation classes are serialized
# process-wide: any number of concurrent captures OR any number of
# concurrent unsafe host-memory ops, never both. Captures are ~ms and
# uploads ~10-100 ms, so the serialization cost is noise next to the
# ~50-100 ms saved per duplicate-content cold load by the blob cache.
# ---------------------------------------------------------------------------
class _CaptureGuard:
    def __init__(self):
        import os as _os
        self._cv = threading.Condition()
        self._captures = 0
        self._unsafe = 0
        self._unsafe_waiting = 0
        self.enabled = _os.environ.get(
            "TFSC_CAPTURE_GUARD", "on").lower() not in ("off", "0", "no")

    def _waited(self, t0: float, what: str) -> None:
        import time as _time
        dt = _time.monotonic() - t0
        if dt > 0.25:
            log.warning("capture-guard: %s waited %.2fs "
                        "(captures=%d unsafe=%d)", what, dt,
                        self._captures, self._unsafe)

    @contextlib.contextmanager
    def capture(self):
        if not self.enabled:
            yield
            return
        import time as _time
        t0 = _time.monotonic()
        with self._cv:
            # writer preference: a QUEUED unsafe op blocks new captures
            # too, so an upload waits out at most the captures already
            # in flight (a few ms) instead of a continuous stream of
            # them (measured ~40 ms per cold load under LRU churn)
            while self._unsafe or self._unsafe_waiting:
                self._cv.wait()
            self._captures += 1
        self._waited(t0, "capture")
        try:
            yield
        finally:
            with self._cv:
                self._captures -= 1
                self._cv.notify_all()

    @contextlib.contextmanager
    def unsafe_host_op(self):
        if not self.enabled:
            yield
            return
        import time as _time
        t0 = _time.monotonic()
        with self._cv:
            self._unsafe_waiting += 1
            try:
                while self._captures:
                    self._cv.wait()
                self._unsafe += 1
            finally:
                self._unsafe_waiting -= 1
        self._waited(t0, "unsafe-host-op")
        try:
            yield
        finally:
            with self._cv:
                self._unsafe -= 1
                self._cv.notify_all()


capture_guard = _CaptureGuard()


# converted-weight cache: pinned bf16 blobs keyed by Plan identity.
# Plans are content-deduplicated (engine/model.py inode-keyed plan
# cache), so models sharing a SavedModel's bytes share a Plan — their
# cold loads skip the CPU f32->bf16 convert and become one DMA.
# Bounded: ~51 MB pinned per ResNet-50-sized plan.
_BLOB_CACHE_CAP = 4
_blob_cache_lock = threading.Lock()
_blob_cache: Dict[int, tuple] = {}       # id(plan) -> (plan, blob)
_blob_cache_order: List[int] = []
# single-flight for the CPU convert: concurrent first loads of one
# content must not both run the (expensive, device-synchronizing)
# convert path — the loser waits and takes the cached blob
_convert_locks: Dict[int, threading.Lock] = {}


def _convert_lock(plan) -> threading.Lock:
    with _blob_cache_lock:
        lk = _convert_locks.get(id(plan))
        if lk is None:
            lk = threading.Lock()
            _convert_locks[id(plan)] = lk
            while len(_convert_locks) > 4 * _BLOB_CACHE_CAP:
                _convert_locks.pop(next(iter(_convert_locks)))
        return lk


def _blob_cache_get(plan):
    with _blob_cache_lock:
        ent = _blob_cache.get(id(plan))
        if ent is None or ent[0] is not plan:
            return None
        _blob_cache_order.remove(id(plan))
        _blob_cache_order.append(id(plan))
        return ent[1]


def _blob_cache_put(plan, blob) -> None:
    with _blob_cache_lock:
        key = id(plan)
        if key not in _blob_cache:
            _blob_cache_order.append(key)
        # keep the Plan object referenced so id() stays unambiguous
        _blob_cache[key] = (plan, blob)
        while len(_blob_cache_order) > _BLOB_CACHE_CAP:
            old = _blob_cache_order.pop(0)
            _blob_cache.pop(old, None)


# ---------------------------------------------------------------------------
# pinned host-buffer pool. Every cold load used to hipHostMalloc (and
# every eviction hipHostFree) ~10 MB of per-context staging buffers —
# milliseconds per call, and host allocs during another thread's
# capture are exactly the unsafe ops the capture guard serializes.
# Recycling them removes both costs from the LRU churn path.
# ---------------------------------------------------------------------------
class _PinnedPool:
    KLASS = 1 << 20                 # size classes of 1 MiB

    def __init__(self, cap_bytes: int = 2 << 30):
        self._lock = threading.Lock()
        self._free: Dict[int, List[object]] = {}
        self._pooled = 0
        self.cap = cap_bytes

    def _klass(self, nbytes: int) -> int:
        return max(1, (nbytes + self.KLASS - 1) // self.KLASS) * self.KLASS

    def alloc(self, torch, nbytes: int):
        """Raw pinned uint8 tensor of at least nbytes (class-rounded)."""
        k = self._klass(nbytes)
        with self._lock:
            lst = self._free.get(k)
            if lst:
                self._pooled -= k
                return lst.pop()
        with capture_guard.unsafe_host_op():
            return torch.empty(k, dtype=torch.uint8, pin_memory=True)

    def free(self, raw) -> None:
        if raw is None:
            return
        k = raw.numel()
        with self._lock:
            if self._pooled + k > self.cap:
                return              # drop (freed by GC outside the pool)
            self._free.setdefault(k, []).append(raw)
            self._pooled += k


pinned_pool = _PinnedPool()


def _pin_view(torch, raw, shape, dtype):
    n = int(np.prod(shape)) if shape else 1
    esz = torch.tensor([], dtype=dtype).element_size()
    return raw[:n * esz].view(dtype).view(shape)


# dedicated per-device upload streams: the cached-blob DMA must not run
# on the default (legacy) stream, whose implicit cross-stream semantics
# interact with capturing streams
_upload_streams: Dict[str, object] = {}
_upload_streams_lock = threading.Lock()


def _get_upload_stream(torch, device: str):
    with _upload_streams_lock:
        s = _upload_streams.get(device)
        if s is None:
            s = torch.cuda.Stream(device=device)
            _upload_streams[device] = s
        return s


# ---------------------------------------------------------------------------
# plan-level context templates + transform arenas.
#
# Under the 1000-model LRU workload, models sharing a SavedModel's bytes
# share a Plan (inode-keyed plan cache) — yet every cold load re-ran the
# Python-heavy buffer planning, call emission and per-layer weight
# transforms, and under GIL contention with the serving threads that
# Python work WAS the cold-load cost. Both are plan-deterministic:
#
#  * the CONTEXT TEMPLATE (engine/emit.py) holds shapes/roots/buffer
#    offsets/scratch and the kernel calls with every pointer written as
#    (region key, offset); every context is instantiated from it by
#    pure pointer relocation, and models sharing the plan share it;
#  * the TRANSFORM ARENA caches the transformed weight bytes
#    (pre-transposed GEMM/conv layouts, fp8 quantized weights) in
#    pinned host memory; a new model restores them with ONE DMA into a
#    device arena and views at recorded offsets — no per-layer
#    transform compute, and every transform lands at a deterministic
#    arena offset (which is what makes call relocation possible).
# ---------------------------------------------------------------------------
_TMPL_CAP = 64          # templates are ~100 KB of host data each
_ARENA_CAP = 4          # arenas pin ~50 MB of host RAM each (like the
                        # blob cache: only the hottest plan contents)
_tmpl_lock = threading.Lock()
_ctx_templates: Dict[tuple, tuple] = {}     # (id(plan),bucket,dtype) ->
                                            # (plan, (Template,
                                            #         ext.CallTemplate))
_tmpl_order: List[tuple] = []
_transform_arenas: Dict[tuple, tuple] = {}  # (id(plan),dtype) ->
                                            # (plan, entries, pinned)
_arena_order: List[tuple] = []


def _get_ctx_template(plan, bucket: int, dtype: str):
    with _tmpl_lock:
        key = (id(plan), bucket, dtype)
        ent = _ctx_templates.get(key)
        if ent is None or ent[0] is not plan:
            return None
        _tmpl_order.remove(key)
        _tmpl_order.append(key)
        return ent[1]


def _put_ctx_template(plan, bucket: int, dtype: str, tmpl) -> None:
    with _tmpl_lock:
        key = (id(plan), bucket, dtype)
        if key not in _ctx_templates:
            _tmpl_order.append(key)
        _ctx_templates[key] = (plan, tmpl)
        while len(_tmpl_order) > _TMPL_CAP:
            old = _tmpl_order.pop(0)
            _ctx_templates.pop(old, None)


def _get_transform_arena(plan, dtype: str):
    with _tmpl_lock:
        key = (id(plan), dtype)
        ent = _transform_arenas.get(key)
        if ent is None or ent[0] is not plan:
            return None
        _arena_order.remove(key)
        _arena_order.append(key)
        return ent[1], ent[2]


def _put_transform_arena(plan, dtype: str, entries, pinned) -> None:
    with _tmpl_lock:
        key = (id(plan), dtype)
        if key in _transform_arenas:
            return
        _arena_order.append(key)
        _transform_arenas[key] = (plan, entries, pinned)
        while len(_arena_order) > _ARENA_CAP:
            old = _arena_order.pop(0)
            _transform_arenas.pop(old, None)


def _call_template(ext, tmpl):
    """The C++ form of a template's calls: kinds by the extension's
    K_* value, pointers as (0, off) workspace | (1, region index, off)
    | (2,) null."""
    index = {k: i for i, k in enumerate(tmpl.region_keys)}
    return ext.CallTemplate([
        (getattr(ext, "K_" + kind),
         [(2,) if d is None else (0, d[1]) if d[0] == WS
          else (1, index[d[0]], d[1]) for d in descs],
         ints, floats)
        for kind, descs, ints, floats in tmpl.calls])


class ExecContext:
    """Shapes + workspace + calls for one batch bucket."""

    def __init__(self, gm: "GpuModel", batch: int):
        self.gm = gm
        self.batch = batch
        torch, ext = _load_backend()
        plan = gm.plan
        dev = gm.device

        # all the Python-heavy planning and emission is done once per
        # (plan, bucket, dtype); a context is the template plus device
        # memory: allocate the workspace, resolve the template's weight
        # regions to base addresses and rebase the calls (one pybind
        # call)
        cached = _get_ctx_template(plan, batch, gm.dtype)
        if cached is None:
            tmpl = build_template(plan, batch, gm.dtype)
            ctmpl = _call_template(ext, tmpl)
        else:
            tmpl, ctmpl = cached
        self.shapes = tmpl.shapes
        self.root = tmpl.root
        self.bufs = tmpl.bufs
        self.total_bytes = tmpl.total_bytes
        self.scratch_off = tmpl.scratch_off
        self.workspace = torch.empty(self.total_bytes,
                                     dtype=torch.uint8, device=dev)
        n_before = gm.n_transforms()
        bases = gm.region_bases(tmpl.region_keys)
        self.exec_plan = ext.instantiate_plan(
            ctmpl, self.workspace.data_ptr(), bases)
        # a context whose template was cached and whose transforms all
        # existed needs no eager warm-up run before capture (prewarm)
        self._from_template = cached is not None and \
            gm.n_transforms() == n_before
        if cached is None:
            _put_ctx_template(plan, batch, gm.dtype, (tmpl, ctmpl))
            # the template's region keys must be resolvable by later
            # models sharing the plan — snapshot the transform bytes now
            gm.publish_transform_arena()
        self.captured = False
        self._views: Dict[int, object] = {}
        self.lock = threading.Lock()
        self.fast_id: Optional[int] = None   # set once fast-registered
        # dedicated non-default stream (the default stream cannot be
        # hipGraph-captured; copies + kernels + D2H all run here)
        self.stream = torch.cuda.Stream(device=dev)
        # pinned host staging per feed/fetch tensor: numpy -> pinned
        # (with dtype conversion on CPU) -> one async DMA, instead of a
        # pageable f32 copy + on-device convert per request
        self._pinned_in: Dict[int, object] = {}
        self._pinned_out: Dict[int, object] = {}
        self._pin_raws: List[object] = []   # pooled pinned backings

    def capture_only(self):
        """Capture the hipGraph WITHOUT an eager warm-up run: valid
        for contexts whose template was cached and whose transforms
        all existed (_from_template; the warm-up run existed to flush
        lazy allocations before capture). Saves a full model execution
        per cold load under LRU churn."""
        torch, _ = _load_backend()
        with torch.cuda.device(self.gm.device), \
                torch.cuda.stream(self.stream):
            try:
                with capture_guard.capture():
                    self.exec_plan.capture()
            except Exception:       # noqa: BLE001
                log.exception("hipGraph capture failed; staying eager")
            self.captured = True

    # -- runtime -----------------------------------------------------------
    def view(self, idx: int):
        torch, _ = _load_backend()
        r = self.root[idx]
        v = self._views.get(idx)
        if v is not None:
            return v
        info = self.bufs[r]
        t = self.gm.plan.tensors[r]
        base = self.workspace[info.offset:info.offset + info.nbytes]
        if t.dtype == "i32":
            v = base.view(torch.int32)[:int(np.prod(self.shapes[idx]))]
        else:
            v = base.view(torch.bfloat16)[:int(np.prod(self.shapes[idx]))]
        v = v.view(self.shapes[idx])
        self._views[idx] = v
        return v

    def run(self, feeds: Dict[int, np.ndarray],
            fetch: List[int]) -> Dict[int, np.ndarray]:
        # once fast-registered, the C++ per-context mutex is the lock for
        # this context's stream/buffers — take it so the Python and C++
        # paths serialize against each other
        if self.fast_id is not None and self.fast_id >= 0:
            self.gm._fast.lock_ctx(self.fast_id)
            try:
                return self._run_inner(feeds, fetch)
            finally:
                self.gm._fast.unlock_ctx(self.fast_id)
        return self._run_inner(feeds, fetch)

    def _run_inner(self, feeds: Dict[int, np.ndarray],
                   fetch: List[int]) -> Dict[int, np.ndarray]:
        torch, _ = _load_backend()
        with torch.cuda.device(self.gm.device), \
                torch.cuda.stream(self.stream):
            for idx, arr in feeds.items():
                v = self.view(idx)
                pin = self._pinned_in.get(idx)
                if pin is None or pin.shape != v.shape:
                    raw = pinned_pool.alloc(
                        torch, int(np.prod(v.shape)) * v.element_size())
                    self._pin_raws.append(raw)
                    pin = _pin_view(torch, raw, tuple(v.shape), v.dtype)
                    self._pinned_in[idx] = pin
                if hasattr(arr, "segments"):
                    # segmented batch: copy each request's rows straight
                    # into pinned staging (skips np.concatenate)
                    r0 = 0
                    for seg in arr.segments:
                        t = torch.from_numpy(np.ascontiguousarray(seg))
                        pin[r0:r0 + seg.shape[0]].copy_(t)
                        r0 += seg.shape[0]
                    if r0 < v.shape[0]:
                        pin[r0:].zero_()
                else:
                    t = torch.from_numpy(np.ascontiguousarray(arr))
                    rows = t.shape[0] if t.ndim else 0
                    if t.ndim and rows < v.shape[0]:
                        pin[:rows].copy_(t)      # CPU-side dtype convert
                        pin[rows:].zero_()
                    else:
                        pin.copy_(t.reshape(v.shape))
                v.copy_(pin, non_blocking=True)
            if self.gm.use_graphs and not self.captured:
                # warm-up eager run, then capture on this stream
                # (serialized against unsafe host-memory ops — see
                # capture_guard)
                self.exec_plan.run()
                self.stream.synchronize()
                try:
                    with capture_guard.capture():
                        self.exec_plan.capture()
                except Exception:       # noqa: BLE001
                    log.exception("hipGraph capture failed; staying eager")
                self.captured = True
            if self.captured and self.exec_plan.has_graph():
                self.exec_plan.run_graph()
            else:
                self.exec_plan.run()
            for idx in fetch:
                v = self.view(idx)
                po = self._pinned_out.get(idx)
                if po is None or po.shape != v.shape:
                    dt = (torch.float32 if v.dtype == torch.bfloat16
                          else v.dtype)
                    raw = pinned_pool.alloc(
                        torch, int(np.prod(v.shape)) *
                        torch.tensor([], dtype=dt).element_size())
                    self._pin_raws.append(raw)
                    po = _pin_view(torch, raw, tuple(v.shape), dt)
                    self._pinned_out[idx] = po
                po.copy_(v, non_blocking=True)
            self.stream.synchronize()
            return {idx: self._pinned_out[idx].numpy().copy()
                    for idx in fetch}


class GpuModel:
    """A plan resident on one GPU (weights in HBM + per-bucket contexts)."""

    BUCKETS = (1, 2, 4, 8, 16, 32, 64)

    def __init__(self, plan: Plan, device: str = "cuda:0",
                 max_batch: int = 64, use_graphs: bool = True,
                 n_streams: int = 6, model_name: str = "",
                 model_version: int = 0, dtype: str = "bf16"):
        torch, ext = _load_backend()
        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"engine dtype {dtype!r} (bf16|fp8)")
        self.dtype = dtype
        self.plan = plan
        self.device = device
        self.model_name = model_name
        self.model_version = model_version
        # up to n_streams ExecContexts per batch bucket, each with its
        # own HIP stream + workspace: concurrent requests overlap one
        # context's H2D/D2H with another's kernels
        self.n_streams = max(1, n_streams)
        # C++ fast predict path (request bytes in, response bytes out);
        # contexts register after their first Python-path run + capture
        self._fast = ext.FastModel(model_name or "model",
                                   int(model_version), self.n_streams)
        self.max_batch = max_batch
        self.use_graphs = use_graphs
        self._weights: Dict[int, object] = {}
        self._gemm_weights: Dict[Tuple[int, bool], object] = {}
        self._gemm_weights_fp8: Dict[Tuple[int, bool], tuple] = {}
        self._conv_weights: Dict[int, object] = {}
        self._contexts: Dict[int, List[ExecContext]] = {}
        self._lock = threading.Lock()
        self._released = False
        import os as _os
        import time as _time
        t0 = _time.monotonic()
        self._upload_pending = False
        with torch.cuda.device(device):
            self._upload_weights()
            restored = self.try_restore_transforms()
            if self._upload_pending or restored:
                # one sync covers both async DMAs (master blob +
                # transform arena) on the shared upload stream. MUST be
                # guard-serialized: a stream sync concurrent with
                # another thread's capture invalidates the capture (the
                # 100-step soak reproduced hipErrorStreamCapture*
                # within seconds when this ran unguarded)
                with capture_guard.unsafe_host_op():
                    _get_upload_stream(torch, device).synchronize()
        if _os.environ.get("TFSC_LOAD_TIMING"):
            log.warning("upload_weights %.1fms (cached_blob=%s "
                        "arena=%s)", (_time.monotonic() - t0) * 1e3,
                        _blob_cache_get(plan) is not None, restored)

    # -- weights -----------------------------------------------------------
    def _upload_weights(self) -> None:
        """One coalesced H2D for all float weights: each is converted to
        bf16 into a single pinned buffer (vectorized CPU convert), then
        ONE DMA moves the model; per-tensor views slice the device blob.
        (~270 individual .to(device) calls cost 60-130 ms per ResNet-50
        cold load; this path is ~10 ms + one 100 MB transfer.)"""
        torch, _ = _load_backend()
        # the same layout call emission addresses the blob by
        layout = blob_layout(self.plan)
        tensors = self.plan.tensors
        self._int_idx = layout.int_idx
        for idx in layout.int_idx:
            self._weights[idx] = torch.from_numpy(np.ascontiguousarray(
                tensors[idx].weight.astype(np.int32))).to(self.device)
        float_ws = [(idx, tensors[idx].weight, off, n)
                    for idx, (off, n) in layout.slots.items()]
        total = layout.total
        if not float_ws:
            return
        import os as _os
        import time as _time
        timing = _os.environ.get("TFSC_LOAD_TIMING")
        ta = _time.monotonic()
        blob = torch.empty(total, dtype=torch.bfloat16, device=self.device)
        tb = _time.monotonic()
        cached = _blob_cache_get(self.plan)
        conv_held = False
        conv_lock = None
        if cached is None:
            # single-flight the convert; a second concurrent first-load
            # of the same content waits and takes the cached blob
            conv_lock = _convert_lock(self.plan)
            conv_lock.acquire()
            conv_held = True
            cached = _blob_cache_get(self.plan)
            if cached is not None:
                conv_lock.release()
                conv_held = False
        try:
            self._upload_blob(torch, blob, cached, total, float_ws,
                              timing, ta, tb)
        finally:
            if conv_held:
                conv_lock.release()

    def _upload_blob(self, torch, blob, cached, total, float_ws,
                     timing, ta, tb):
        import time as _time
        if cached is not None and cached.numel() == total:
            # converted blob already pinned in CPU RAM: ONE DMA on the
            # dedicated upload stream, guard-serialized against captures
            # (running it unguarded produced
            # hipErrorStreamCaptureInvalidated under the full headline
            # workload; the guard's writer preference keeps the wait to
            # the captures already in flight, a few ms)
            up = _get_upload_stream(torch, self.device)
            tc = _time.monotonic()
            with capture_guard.unsafe_host_op():
                td = _time.monotonic()
                with torch.cuda.stream(up):
                    blob.copy_(cached, non_blocking=True)
                te = _time.monotonic()
                up.synchronize()
            if timing:
                tf_ = _time.monotonic()
                log.warning(
                    "upload phases: alloc=%.1f guard=%.1f copy=%.1f "
                    "sync=%.1f ms", (tb - ta) * 1e3, (td - tc) * 1e3,
                    (te - td) * 1e3, (tf_ - te) * 1e3)
        else:
            # stage through a SHARED reusable pinned buffer: per-load
            # pinned allocation (page-locking ~100 MB) costs more than
            # the copy and thrashes badly under LRU churn. The converted
            # result is ALSO written to a cacheable pinned blob so the
            # next load of this plan skips the CPU convert entirely.
            cpu_blob = None
            try:
                with capture_guard.unsafe_host_op():
                    cpu_blob = torch.empty(total, dtype=torch.bfloat16,
                                           pin_memory=True)
            except RuntimeError:
                log.warning("pinned weight-blob allocation failed; "
                            "skipping the converted-weight cache")
            # the convert's flush() does DEVICE-WIDE synchronizes —
            # unguarded, those poison any concurrent hipGraph capture
            # (reproduced by the 2-rank-on-one-GPU dry run), so the
            # whole staging loop is an unsafe host op. It runs once per
            # plan content (single-flighted above).
            with capture_guard.unsafe_host_op(), _staging_lock:
                stage = _get_staging(torch)
                cap = stage.numel()
                batch_items = []        # (stage_off, blob_off, n)
                stage_off = 0

                def flush():
                    nonlocal stage_off
                    for s_off, b_off, n_ in batch_items:
                        blob[b_off:b_off + n_].copy_(
                            stage[s_off:s_off + n_], non_blocking=True)
                    torch.cuda.synchronize(self.device)
                    batch_items.clear()
                    stage_off = 0

                for _idx, w, off, n in float_ws:
                    src = torch.from_numpy(np.ascontiguousarray(
                        np.asarray(w, dtype=np.float32))).view(-1)
                    done = 0
                    while done < n:
                        if stage_off >= cap:
                            flush()
                        take = min(n - done, cap - stage_off)
                        stage[stage_off:stage_off + take].copy_(
                            src[done:done + take])  # CPU f32->bf16
                        if cpu_blob is not None:
                            cpu_blob[off + done:off + done + take].copy_(
                                stage[stage_off:stage_off + take])
                        batch_items.append((stage_off, off + done, take))
                        stage_off += take
                        done += take
                flush()
            if cpu_blob is not None:
                _blob_cache_put(self.plan, cpu_blob)
        self._weight_blob = blob              # keep the allocation alive
        # LAZY views: ~270 torch view creations per cold load cost
        # milliseconds; master_weight materializes on demand (a context
        # addresses the blob by offset and needs no view)
        self._blob_slots = {idx: (off, n, tuple(w.shape))
                            for idx, w, off, n in float_ws}

    def master_weight(self, idx: int):
        """bf16 master view of plan weight idx (blob slice or int
        tensor), materialized lazily."""
        t = self._weights.get(idx)
        if t is not None:
            return t
        slot = getattr(self, "_blob_slots", {}).get(idx)
        if slot is None:
            raise KeyError(f"no master weight for tensor {idx}")
        off, n, shape = slot
        t = self._weight_blob[off:off + n].view(shape)
        self._weights[idx] = t
        return t

    def has_master_weight(self, idx: int) -> bool:
        return idx in self._weights or \
            idx in getattr(self, "_blob_slots", {})

    def zeros_ptr(self) -> int:
        """A small zeroed device buffer used as the gather source for
        out-of-image conv patches (csrc/ops/gemm.hip stage_tile_conv_a)."""
        torch, _ = _load_backend()
        if getattr(self, "_zeros", None) is None:
            self._zeros = torch.zeros(64, dtype=torch.uint8,
                                      device=self.device)
        return self._zeros.data_ptr()

    def gemm_weight(self, idx: int, graph_trans_b: bool):
        """[N][Kpad] bf16 pre-transposed weight for the GEMM kernel."""
        torch, _ = _load_backend()
        key = (idx, graph_trans_b)
        wt = self._gemm_weights.get(key)
        if wt is not None:
            return wt
        av = self._arena_view(("gw",) + key)
        if av is not None:
            self._gemm_weights[key] = av
            return av
        if not self.has_master_weight(idx):
            raise RuntimeError(
                "GPU gemm requires a constant weight operand; "
                "activation x activation MatMul must be BatchMatMul")
        w = self.master_weight(idx).float()
        if not graph_trans_b:
            w = w.t().contiguous()      # [K,N] -> [N,K]
        N, K = w.shape
        Kp = _pad64(K)
        if Kp != K:
            w = torch.nn.functional.pad(w, (0, Kp - K))
        wt = w.to(torch.bfloat16).contiguous()
        self._gemm_weights[key] = wt
        return wt

    def gemm_weight_fp8(self, idx: int, graph_trans_b: bool):
        """(e4m3 [N][Kp128] bytes, f32 [N] per-output-channel scales)
        for the fp8 GEMM: amax/448 per row of the pre-transposed weight
        (the standard rowwise fp8 serving recipe; dequant happens in the
        kernel's f32 epilogue)."""
        torch, _ = _load_backend()
        key = (idx, graph_trans_b)
        ent = self._gemm_weights_fp8.get(key)
        if ent is not None and ent[0] is not None and \
                ent[1] is not None:
            return ent
        q_av = self._arena_view(("f8q",) + key)
        s_av = self._arena_view(("f8s",) + key)
        if q_av is not None and s_av is not None:
            self._gemm_weights_fp8[key] = (q_av, s_av)
            return q_av, s_av
        if not self.has_master_weight(idx):
            raise RuntimeError("fp8 gemm requires a constant weight")
        w = self.master_weight(idx).float()
        if not graph_trans_b:
            w = w.t().contiguous()          # [K,N] -> [N,K]
        N, K = w.shape
        amax = w.abs().amax(dim=1).clamp(min=1e-12)
        scale = (amax / 448.0).to(torch.float32).contiguous()
        q = (w / scale[:, None]).clamp(-448.0, 448.0).to(
            torch.float8_e4m3fn).view(torch.uint8)
        Kp = _pad128(K)
        if Kp != K:
            q = torch.nn.functional.pad(q, (0, Kp - K))
        q = q.contiguous()
        ent = (q, scale)
        self._gemm_weights_fp8[key] = ent
        return ent

    def conv_weight(self, idx: int):
        """[Kc][pad64(R*S*C)] bf16 from the [R,S,C,K] master."""
        torch, _ = _load_backend()
        wt = self._conv_weights.get(idx)
        if wt is not None:
            return wt
        av = self._arena_view(("cw", idx))
        if av is not None:
            self._conv_weights[idx] = av
            return av
        w = self.master_weight(idx).float()     # [R,S,C,K]
        R, S, C, Kc = w.shape
        w = w.reshape(R * S * C, Kc).t().contiguous()   # [K][RSC]
        Kp = _pad64(R * S * C)
        if Kp != R * S * C:
            w = torch.nn.functional.pad(w, (0, Kp - R * S * C))
        wt = w.to(torch.bfloat16).contiguous()
        self._conv_weights[idx] = wt
        return wt

    def conv_weight_cpad(self, idx: int, c8: int):
        """[Kc][pad64(R*S*c8)] bf16 with the input-channel dim widened to
        c8 (zeros) — pairs with the K_PAD_LAST channel widening."""
        torch, _ = _load_backend()
        key = (idx, "cpad", c8)
        wt = self._conv_weights.get(key)
        if wt is not None:
            return wt
        av = self._arena_view(("cw",) + key)
        if av is not None:
            self._conv_weights[key] = av
            return av
        w = self.master_weight(idx).float()     # [R,S,C,K]
        R, S, C, Kc = w.shape
        w = torch.nn.functional.pad(w, (0, 0, 0, c8 - C))  # pad C dim
        w = w.reshape(R * S * c8, Kc).t().contiguous()
        Kp = _pad64(R * S * c8)
        if Kp != R * S * c8:
            w = torch.nn.functional.pad(w, (0, Kp - R * S * c8))
        wt = w.to(torch.bfloat16).contiguous()
        self._conv_weights[key] = wt
        return wt

    # -- transform arena / relocation regions ------------------------------
    def _region_items(self):
        """[(key, tensor)] of the weight regions the transform arena
        snapshots: int weights and every materialised transform."""
        items = []
        for idx in getattr(self, "_int_idx", []):
            items.append((("int", idx), self._weights[idx]))
        for k, t in self._gemm_weights.items():
            items.append((("gw",) + k, t))
        for k, t in self._conv_weights.items():
            kk = k if isinstance(k, tuple) else (k,)
            items.append((("cw",) + kk, t))
        for k, (q, sc) in self._gemm_weights_fp8.items():
            items.append((("f8q",) + tuple(k), q))
            items.append((("f8s",) + tuple(k), sc))
        return items

    def n_transforms(self) -> int:
        """How many weight transforms this model holds as tensors."""
        return len(self._gemm_weights) + len(self._conv_weights) + \
            len(self._gemm_weights_fp8)

    def region_bases(self, keys) -> List[int]:
        """Device base address of each weight region a call template
        names by key (engine/emit.py lists the keys). A region comes
        from the restored arena when the model has one (one dict lookup
        per key: this runs on every cold load), else from _region_ptr."""
        arena = getattr(self, "_arena_dev", None)
        entries = self._arena_entries if arena is not None else {}
        arena_base = arena.data_ptr() if arena is not None else 0
        bases = []
        for key in keys:
            ent = entries.get(key)
            bases.append(arena_base + ent[1] if ent is not None
                         else self._region_ptr(key))
        return bases

    def _region_ptr(self, key: tuple) -> int:
        """A region outside the arena; a transform is materialised on
        demand."""
        kind = key[0]
        if kind == "blob":
            return self._weight_blob.data_ptr()
        if kind == "zeros":
            return self.zeros_ptr()
        if kind == "int":
            return self._weights[key[1]].data_ptr()
        if kind == "gw":
            return self.gemm_weight(key[1], key[2]).data_ptr()
        if kind == "cw" and len(key) == 2:
            return self.conv_weight(key[1]).data_ptr()
        if kind == "cw" and key[2] == "cpad":
            return self.conv_weight_cpad(key[1], key[3]).data_ptr()
        if kind in ("f8q", "f8s"):
            q, scale = self.gemm_weight_fp8(key[1], key[2])
            return (q if kind == "f8q" else scale).data_ptr()
        raise KeyError(f"unknown weight region {key}")

    def publish_transform_arena(self) -> None:
        """Snapshot this model's transformed weights into a pinned host
        arena keyed by the (content-deduplicated) plan, so later models
        restore them with one DMA instead of per-layer transforms."""
        torch, _ = _load_backend()
        if _get_transform_arena(self.plan, self.dtype) is not None:
            return
        items = self._region_items()
        entries = []
        off = 0
        for key, t in items:
            nb = t.numel() * t.element_size()
            entries.append((key, off, nb, t.dtype, tuple(t.shape)))
            off = _pad256b(off + nb)
        if off == 0:
            return
        try:
            with capture_guard.unsafe_host_op():
                pinned = torch.empty(off, dtype=torch.uint8,
                                     pin_memory=True)
        except RuntimeError:
            log.warning("pinned transform-arena alloc failed; later "
                        "models will re-transform")
            return
        for (key, o, nb, dt, shape), (_k, t) in zip(entries, items):
            pinned[o:o + nb].view(dt)[:t.numel()].copy_(
                t.reshape(-1), non_blocking=False)
        _put_transform_arena(self.plan, self.dtype, entries, pinned)

    def try_restore_transforms(self) -> bool:
        """One DMA restore of the transformed weights from the plan's
        pinned arena (replaces the per-layer GPU transforms on repeat
        cold loads of the same content)."""
        torch, _ = _load_backend()
        got = _get_transform_arena(self.plan, self.dtype)
        if got is None:
            return False
        entries, pinned = got
        dev_arena = torch.empty(pinned.numel(), dtype=torch.uint8,
                                device=self.device)
        up = _get_upload_stream(torch, self.device)
        with capture_guard.unsafe_host_op():
            with torch.cuda.stream(up):
                dev_arena.copy_(pinned, non_blocking=True)
        self._arena_dev = dev_arena
        # LAZY views: region_bases() computes pointers straight from
        # the entry offsets; tensor views materialize only if someone
        # asks an accessor for the transform itself. ~300 eager view
        # creations per cold load were milliseconds of Python.
        self._arena_entries = {tuple(e[0]): e for e in entries}
        # int weights live in the arena from here on (master_weight
        # reads _weights[idx]); they are few
        for key, off, nb, dt, shape in entries:
            if key[0] == "int":
                self._weights[key[1]] = \
                    dev_arena[off:off + nb].view(dt).view(shape)
        return True

    def _arena_view(self, key: tuple):
        ent = getattr(self, "_arena_entries", {}).get(tuple(key))
        if ent is None or self._arena_dev is None:
            return None
        _key, off, nb, dt, shape = ent
        return self._arena_dev[off:off + nb].view(dt).view(shape)

    def weight_bytes(self) -> int:
        total = 0
        blob = getattr(self, "_weight_blob", None)
        if blob is not None:
            total += blob.numel() * blob.element_size()
        arena = getattr(self, "_arena_dev", None)
        if arena is not None:
            total += arena.numel() * arena.element_size()
        for d in (self._weights, self._gemm_weights, self._conv_weights):
            for wt in d.values():
                if wt is not None and getattr(wt, "untyped_storage",
                                              None) is not None:
                    total += wt.numel() * wt.element_size()
        return total

    # -- execution ---------------------------------------------------------
    def _bucket(self, batch: int) -> int:
        for b in self.BUCKETS:
            if b >= batch and b <= self.max_batch:
                return b
        return self.max_batch

    def streams_for(self, bucket: int) -> int:
        # small batches under-fill the chip AND have cheap workspaces:
        # give them proportionally more concurrent contexts
        if bucket <= 4:
            return self.n_streams * 2
        return self.n_streams

    def _acquire_context(self, batch: int) -> ExecContext:
        """Returns a LOCKED ExecContext for the bucket: an idle one if
        available, a freshly built one while under the bucket's stream
        budget, else blocks on the least-loaded."""
        b = self._bucket(batch)
        with self._lock:
            if self._released:
                raise ModelReleasedError(
                    "model was evicted from the GPU pool")
            ctxs = self._contexts.setdefault(b, [])
            for ctx in ctxs:
                if ctx.lock.acquire(blocking=False):
                    return ctx
            if len(ctxs) < self.streams_for(b):
                ctx = ExecContext(self, b)
                ctxs.append(ctx)
                ctx.lock.acquire()
                return ctx
            ctx = ctxs[0]
        ctx.lock.acquire()
        return ctx

    def run(self, feeds: Dict[int, np.ndarray], batch: int,
            fetch: List[int]) -> Dict[int, np.ndarray]:
        if self._released:
            raise ModelReleasedError("model was evicted from the GPU pool")
        ctx = self._acquire_context(batch)
        try:
            if self._released:
                raise ModelReleasedError(
                    "model was evicted from the GPU pool")
            out = ctx.run(feeds, fetch)
            # after the first captured run completes (stream idle),
            # expose the context to the C++ fast path
            if ctx.fast_id is None and ctx.captured:
                try:
                    self._register_fast(ctx)
                except Exception:       # noqa: BLE001
                    log.exception("fast-path registration failed")
        finally:
            ctx.lock.release()
        if ctx.batch != batch:
            # un-pad the batch dimension of fetched outputs
            plan = self.plan
            for idx in list(out):
                shape = plan.tensors[idx].shape
                if shape and is_sym(shape[0]):
                    rows = resolve_dim(shape[0], batch)
                    out[idx] = out[idx][:rows]
        return out

    def fast_predict(self, request_bytes: bytes) -> bytes:
        """C++ end-to-end predict (raises ext.FastFallback when the
        request shape/bucket isn't registered yet — callers then take
        the Python path, which builds and registers the context)."""
        if self._released:
            raise ModelReleasedError("model was evicted from the GPU pool")
        return self._fast.predict(request_bytes)

    def _register_fast(self, ctx: "ExecContext") -> None:
        torch, ext = _load_backend()
        plan = self.plan
        keep = []
        ins = []
        for alias, idx in plan.sig_inputs.items():
            v = ctx.view(idx)
            is_int = v.dtype == torch.int32
            rows = v.shape[0] if v.ndim else 1
            row_elems = int(np.prod(v.shape[1:])) if v.ndim > 1 else 1
            raw = pinned_pool.alloc(torch, rows * row_elems * 4)
            ctx._pin_raws.append(raw)
            pin = _pin_view(torch, raw, (rows, row_elems),
                            torch.int32 if is_int else torch.float32)
            if is_int:
                stage_ptr = 0
            else:
                stage = torch.empty((rows, row_elems), dtype=torch.float32,
                                    device=self.device)
                keep.append(stage)
                stage_ptr = stage.data_ptr()
            keep.append(pin)
            ins.append(ext.FastIO(alias, bool(is_int), pin.data_ptr(),
                                  stage_ptr, v.data_ptr(), row_elems,
                                  [int(d) for d in v.shape[1:]]))
        outs = []
        for alias, idx in plan.sig_outputs.items():
            v = ctx.view(idx)
            if v.dtype != torch.bfloat16:
                ctx.fast_id = -1     # non-bf16 output: python path only
                return
            rows = v.shape[0] if v.ndim else 1
            row_elems = int(np.prod(v.shape[1:])) if v.ndim > 1 else 1
            raw = pinned_pool.alloc(torch, rows * row_elems * 4)
            ctx._pin_raws.append(raw)
            pin = _pin_view(torch, raw, (rows, row_elems), torch.float32)
            stage = torch.empty((rows, row_elems), dtype=torch.float32,
                                device=self.device)
            keep.extend([pin, stage])
            outs.append(ext.FastIO(alias, False, pin.data_ptr(),
                                   stage.data_ptr(), v.data_ptr(),
                                   row_elems, [int(d) for d in v.shape[1:]]))
        ctx._fast_keep = keep
        ctx.fast_id = self._fast.add_context(
            ctx.batch, self.streams_for(ctx.batch), ctx.exec_plan.ptr(),
            ctx.stream.cuda_stream, ins, outs)

    def prewarm(self, batch: int, limit: Optional[int] = None) -> None:
        """Build + capture + fast-register the bucket's stream contexts
        with zero feeds (all of them by default; `limit` caps the count
        — LRU-churn loads prewarm ONE context on the loader thread so
        even a model's FIRST request takes the C++ fast path).
        Server-side batching needs the full set: the merged bucket is
        only ever used by the C++ fast path, so the Python path's
        contention-driven context building never reaches it."""
        plan = self.plan
        b = self._bucket(batch)
        want = self.streams_for(b) if limit is None \
            else min(limit, self.streams_for(b))
        feeds = {}
        for _alias, idx in plan.sig_inputs.items():
            shape = plan.resolve_shape(plan.tensors[idx].shape, b)
            dt = np.int32 if plan.tensors[idx].dtype == "i32" \
                else np.float32
            feeds[idx] = np.zeros(shape, dtype=dt)
        fetch = list(plan.sig_outputs.values())
        with self._lock:
            if self._released:
                raise ModelReleasedError(
                    "model was evicted from the GPU pool")
            ctxs = self._contexts.setdefault(b, [])
            while len(ctxs) < want:
                ctxs.append(ExecContext(self, b))
            todo = [c for c in ctxs if c.fast_id is None]
        for ctx in todo:
            with ctx.lock:
                if getattr(ctx, "_from_template", False) and \
                        self.use_graphs and not ctx.captured:
                    ctx.capture_only()
                else:
                    ctx.run(feeds, fetch)
                if ctx.fast_id is None and ctx.captured:
                    self._register_fast(ctx)

    def release(self) -> None:
        # mark released (new runs fail fast; the cache manager
        # re-fetches), then wait for each in-flight context before
        # freeing the weights under it
        with self._lock:
            self._released = True
            ctx_lists = list(self._contexts.values())
            self._contexts.clear()
        try:
            self._fast.disable()     # waits out in-flight fast predicts
        except Exception:       # noqa: BLE001
            pass
        for ctxs in ctx_lists:
            for ctx in ctxs:
                ctx.lock.acquire()
                ctx.lock.release()
                ctx._pinned_in.clear()
                ctx._pinned_out.clear()
                ctx._fast_keep = None
                for raw in ctx._pin_raws:
                    pinned_pool.free(raw)
                ctx._pin_raws = []
        with self._lock:
            self._weights.clear()
            self._gemm_weights.clear()
            self._gemm_weights_fp8.clear()
            self._conv_weights.clear()
            self._arena_dev = None
            self._arena_entries = {}
            self._blob_slots = {}
            self._weight_blob = None

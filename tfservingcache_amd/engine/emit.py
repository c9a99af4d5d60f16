"""Call emission: (Plan, batch bucket, dtype) -> relocatable call template.

Pure Python over the plan: no torch, no GPU, no extension. Every pointer
a kernel call takes is written as a descriptor, never an address:

    None                    null pointer
    (WS, byte offset)       into the context's workspace arena
    (region key, offset)    into a weight region of the model, where the
                            key is one of
        ("blob",)                   bf16 master blob (see blob_layout)
        ("int", idx)                int32 weight tensor idx
        ("gw", idx, trans_b)        pre-transposed GEMM weight
        ("cw", idx)                 conv weight [Kc][pad64(R*S*C)]
                                    (grouped: C is the group's Cg)
        ("cw", idx, "cpad", c8)     conv weight, input channels widened
        ("f8q"|"f8s", idx, trans_b) fp8 GEMM weight bytes / row scales
        ("zeros",)                  small zeroed buffer (conv gather)

engine/gpu.py resolves each region key to a device base address (from
the transform arena, or by materialising the transform) and rebases the
calls in one C++ call. Call kinds are carried by name ("GEMM" for the
extension's K_GEMM); the numeric enum lives in csrc/executor.cpp only.
"""
from __future__ import annotations

from bisect import bisect_right
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from .planner import Plan, PlanOp, conv3d_transpose_taps, lstm_cols

ALIGN = 256  # byte alignment of workspace slices

WS = ("ws",)        # descriptor key of the workspace arena

# every call kind emission can produce (names of the extension's K_*)
KINDS = frozenset({
    "ELT_UNARY", "ELT_BINARY", "BN_ACT", "SOFTMAX", "LAYERNORM",
    "MEAN_LAST", "MEAN_MID", "POOL", "TRANSPOSE", "GATHER", "PAD_NHWC",
    "GEMM", "BGEMM", "CONV", "PAD_LAST", "ATTENTION", "DEPTHWISE",
    "GEMM_FP8", "QUANT_FP8", "CAST", "ARGMAX_LAST", "SCATTER", "RESIZE",
    "ZERO_INSERT",
})
# kinds no golden call template (tests/golden/call_templates) holds yet.
# KINDS is exactly the set those templates reach; a kind moves there with
# its golden case. _call accepts both sets, and nothing else reads this one
KINDS_NO_GOLDEN = frozenset({"LSTM", "NMS"})

# plan ops that are one [rows, cols] kernel over the last axis
_ROWWISE = {"softmax": "SOFTMAX", "reduce_mean_last": "MEAN_LAST",
            "argmax_last": "ARGMAX_LAST"}

_ACT_CODE = {"none": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "gelu": 4,
             "relu6": 5}

_ELT_CODE = {
    "add": 0, "sub": 1, "mul": 2, "div": 3, "max": 4, "min": 5,
    "sqdiff": 6, "relu": 7, "tanh": 8, "sigmoid": 9, "erf": 10,
    "sqrt": 11, "rsqrt": 12, "exp": 13, "neg": 14, "square": 15,
    "gelu": 16, "relu6": 17,
}


def _pad64(k: int) -> int:
    return (k + 63) // 64 * 64


def _pad128(k: int) -> int:
    return (k + 127) // 128 * 128


def _pad256b(n: int) -> int:
    return (n + 255) // 256 * 256


def topk_segments(rows: int, cols: int, k: int) -> int:
    """P, the number of segments a top-k call splits every row into
    (csrc/ops/topk.hip: one workgroup per segment, then a merge launch
    over the P*k partial results). One workgroup walks its segment
    serially, so a long row on few workgroups leaves the chip idle; the
    merge reads P*k composites, so P grows as sqrt(cols / k).

    Every limit is the edge of what profiles/topk.md measured, and inside
    them the split won every time: rows of at least 16384 columns,
    k <= 100, segments of at least 2048 columns, at most 256 segments a
    row and rows * P <= 256 (the chip's CUs). Outside them P = 1."""
    if cols < 16384 or k > 100:
        return 1
    P = min(int((cols / k) ** 0.5), cols // 2048, 256 // max(rows, 1), 256)
    if P < 2:
        return 1
    seglen = -(-cols // P)
    return -(-cols // seglen)           # no empty last segment


_REDUCE_CODE = {"mean": 0, "sum": 1, "max": 2, "min": 3, "prod": 4}

# limits of reduce_segments, from profiles/reductions.md
REDUCE_SPLIT_MIN_BYTES = 1 << 16     # least input of one unsplit workgroup
REDUCE_SEG_MIN_BYTES = 1 << 13       # least input one segment reads
REDUCE_MAX_WGS_ROWS = 1024           # inner == 1: four workgroups per CU
REDUCE_MAX_WGS_COLS = 512            # inner > 1: two
REDUCE_MAX_SEGMENTS = 512


def reduce_segments(outer: int, red: int, inner: int) -> int:
    """P, the number of segments a `reduce` call splits the reduced axis
    of its [outer, red, inner] view into (csrc/ops/reduce.hip: one
    workgroup per segment writes an f32 partial, a second launch folds
    the P partials). Unsplit, the call runs `outer` workgroups when
    inner == 1 and up to outer * ceil(inner / 64) otherwise (the column
    kernel narrows its tile to 8 lanes of 8 channels when workgroups are
    few), each walking its whole reduced axis with a few loads in
    flight: a long axis on few workgroups leaves most of the 256 CUs
    idle.

    The split pays for a second launch, so it starts only where one
    workgroup's input reaches REDUCE_SPLIT_MIN_BYTES, keeps every
    segment at REDUCE_SEG_MIN_BYTES or more, and stops at
    REDUCE_MAX_WGS_* workgroups and REDUCE_MAX_SEGMENTS. Every limit is
    where the gain ended, or the edge of what was measured, in
    profiles/reductions.md."""
    tile = 1 if inner == 1 else min(inner, 64)
    wgs = outer * -(-inner // tile)
    wg_bytes = red * tile * 2
    if wg_bytes < REDUCE_SPLIT_MIN_BYTES:
        return 1
    max_wgs = REDUCE_MAX_WGS_ROWS if inner == 1 else REDUCE_MAX_WGS_COLS
    P = min(wg_bytes // REDUCE_SEG_MIN_BYTES, max_wgs // max(wgs, 1),
            REDUCE_MAX_SEGMENTS, red)
    if P < 2:
        return 1
    seglen = -(-red // P)
    return -(-red // seglen)            # no empty last segment


def _numel(shape) -> int:
    return int(np.prod(shape)) if shape else 1


def _rows_cols(shape) -> List[int]:
    return [_numel(shape[:-1]), shape[-1]]


def _strides(shape) -> List[int]:
    """Element strides of a contiguous tensor."""
    st = [1] * len(shape)
    for d in range(len(shape) - 2, -1, -1):
        st[d] = st[d + 1] * shape[d + 1]
    return st


def _act(p: dict) -> int:
    return _ACT_CODE[p.get("act", "none")]


def _off(desc, nbytes: int):
    """desc + nbytes (a pointer into the middle of a buffer)."""
    return (desc[0], desc[1] + nbytes)


@dataclass
class _BufInfo:
    offset: int = -1          # byte offset in workspace
    nbytes: int = 0
    shape: Tuple[int, ...] = ()
    is_int: bool = False


@dataclass
class BlobLayout:
    """Where each weight of a plan lives on the device: float weights
    at an element offset of one bf16 master blob (each slot rounded up
    to 128 elements, which keeps 256-byte alignment), integer weights as
    int32 tensors of their own."""
    slots: Dict[int, Tuple[int, int]]    # tensor idx -> (elem off, n)
    total: int                           # blob length in bf16 elements
    int_idx: List[int]


# dtype objects: comparing a dtype with a scalar type builds a dtype per
# comparison, and blob_layout runs on every model load
_INT_DTYPES = (np.dtype(np.int32), np.dtype(np.int64))


def blob_layout(plan: Plan) -> BlobLayout:
    slots: Dict[int, Tuple[int, int]] = {}
    int_idx: List[int] = []
    total = 0
    for t in plan.tensors:
        if t.kind != "weight" or t.weight is None:
            continue
        if t.weight.dtype in _INT_DTYPES:
            int_idx.append(t.idx)
        else:
            n = int(t.weight.size)
            slots[t.idx] = (total, n)
            total += _pad128(n)
    return BlobLayout(slots, total, int_idx)


@dataclass
class LiveBlobLayout(BlobLayout):
    """blob_layout restricted to the float weights some kernel can read,
    in the same order and with the same slot padding. Call emission keeps
    addressing the full layout; full_starts / compact_starts (element
    offsets of the live slots, ascending, index for index) carry an
    offset of one into the other."""
    full_total: int
    full_starts: List[int]
    compact_starts: List[int]

    def compact_byte_offset(self, full_byte_off: int) -> int:
        """The compact-blob byte offset of a full-blob byte offset. An
        offset into the middle of a slot keeps its distance from the slot
        start. KeyError for an offset outside every live slot."""
        i = bisect_right(self.full_starts, full_byte_off // 2) - 1
        if i >= 0:
            d = full_byte_off - self.full_starts[i] * 2
            end = self.compact_starts[i + 1] if i + 1 < len(
                self.compact_starts) else self.total
            # d == 0: the start of an empty slot is still its start
            if d == 0 or d < (end - self.compact_starts[i]) * 2:
                return self.compact_starts[i] * 2 + d
        raise KeyError(f"blob offset {full_byte_off} is in no live slot")


def live_weights(plan: Plan) -> set:
    """Indices of the tensors a kernel can read as a weight: every input
    of an op and every signature output, and the root of its alias chain.
    What the planner folded away (unfolded conv filters, BatchNorm
    vectors) stays in plan.tensors but is in no op's inputs."""
    live = set()
    for op in plan.ops:
        live.update(op.inputs)
    live.update(plan.sig_outputs.values())
    for i in list(live):
        r, seen = i, 0
        while plan.tensors[r].alias_of is not None and seen < 16:
            r = plan.tensors[r].alias_of
            seen += 1
        live.add(r)
    return live


def live_blob_layout(plan: Plan) -> LiveBlobLayout:
    """The layout the device blob and its pinned host copy are given
    (engine/gpu.py). Integer weights are all kept: they are few."""
    full = blob_layout(plan)
    live = live_weights(plan)
    slots: Dict[int, Tuple[int, int]] = {}
    full_starts: List[int] = []
    compact_starts: List[int] = []
    total = 0
    for idx, (off, n) in full.slots.items():     # ascending offsets
        if idx not in live:
            continue
        slots[idx] = (total, n)
        full_starts.append(off)
        compact_starts.append(total)
        total += _pad128(n)
    return LiveBlobLayout(slots, total, full.int_idx, full.total,
                          full_starts, compact_starts)


# One transform-arena region as a padded 2-D transpose of a blob slot:
# csrc/kernels.h LayoutEntry, field for field (40 bytes, no padding).
LAYOUT_ENTRY_DTYPE = np.dtype([
    ("src_off", "<i8"), ("dst_off", "<i8"), ("rin", "<i4"), ("cin", "<i4"),
    ("c_src", "<i4"), ("c_dst", "<i4"), ("transpose", "<i4"), ("kp", "<i4")])
LAYOUT_TILE = 64


def _layout_entry(plan: Plan, key: tuple, layout: BlobLayout = None):
    """(src_off, rin, cin, c_src, c_dst, transpose, kp, dst_rows) of the
    region `key` when it is a re-layout of a blob slot (the "gw" and "cw"
    regions of engine/gpu.py), else None. src_off is in the coordinates
    of `layout` (default: blob_layout(plan))."""
    if layout is None:
        layout = blob_layout(plan)
    if key[0] not in ("gw", "cw") or key[1] not in layout.slots:
        return None
    shape = tuple(plan.tensors[key[1]].weight.shape)
    src_off = layout.slots[key[1]][0]
    if key[0] == "gw" and len(key) == 3 and len(shape) == 2:
        if key[2]:                      # stored [N, K]: copy, pad K
            rin, cin = shape
            ent = (src_off, rin, cin, 1, 1, 0, _pad64(cin), rin)
        else:                           # [K, N] -> [N][pad64(K)]
            rin, cin = shape
            ent = (src_off, rin, cin, rin, rin, 1, _pad64(rin), cin)
    elif key[0] == "cw" and len(shape) == 4 and len(key) in (2, 4):
        R, S, C, Kc = shape
        rin = R * S * C
        if len(key) == 2:               # [R*S*C, K] -> [K][pad64(R*S*C)]
            ent = (src_off, rin, Kc, rin, rin, 1, _pad64(rin), Kc)
        elif key[2] == "cpad" and key[3] >= C:
            ent = (src_off, rin, Kc, C, key[3], 1,
                   _pad64(R * S * key[3]), Kc)
        else:
            return None
    else:
        return None
    if min(ent[1], ent[2], ent[3]) < 1 or max(ent[1:]) >= 1 << 31:
        return None
    return ent


def weight_layout_table(plan: Plan, entries, layout: BlobLayout = None):
    """The descriptor table of ops/weight_layout.hip for a transform
    arena whose regions are `entries` [(key, byte offset, nbytes, ...)]:
    (table, tile_start, covered). table is a LAYOUT_ENTRY_DTYPE array with
    one row per bf16 region that is a pure re-layout of a blob slot
    (conv_weight, conv_weight_cpad, gemm_weight), tile_start [n + 1] int32
    the prefix sum of their 64x64 destination tiles, covered the set of
    their keys. Regions outside it (int weights, fp8 bytes and scales)
    stay a host copy. Plan-deterministic: shapes and `layout` only, which
    defaults to blob_layout(plan); with live_blob_layout(plan) passed in,
    src_off addresses the compact blob."""
    if layout is None:
        layout = blob_layout(plan)
    rows, starts, covered = [], [0], set()
    for e in entries:
        key, off, nb = tuple(e[0]), e[1], e[2]
        ent = _layout_entry(plan, key, layout)
        if ent is None or ent[7] * ent[6] * 2 != nb:
            continue
        rows.append((ent[0], off) + ent[1:7])
        starts.append(starts[-1] + -(-ent[7] // LAYOUT_TILE) *
                      (ent[6] // LAYOUT_TILE))
        covered.add(key)
    if starts[-1] >= 1 << 31:
        return (np.zeros(0, LAYOUT_ENTRY_DTYPE), np.zeros(1, np.int32),
                set())
    return (np.array(rows, dtype=LAYOUT_ENTRY_DTYPE),
            np.array(starts, dtype=np.int32), covered)


def check_layout_table(table, tile_start, blob_elems: int,
                       arena_bytes: int) -> None:
    """Raises ValueError unless every entry reads inside a blob of
    blob_elems elements, writes inside an arena of arena_bytes bytes
    without touching another entry, and tile_start is the prefix sum of
    the entries' tiles. The kernel trusts its table; this is the check."""
    if len(tile_start) != len(table) + 1 or tile_start[0] != 0:
        raise ValueError("tile_start does not match the table")
    spans = []
    for i, e in enumerate(table):
        rin, cin, kp = int(e["rin"]), int(e["cin"]), int(e["kp"])
        c_src, c_dst = int(e["c_src"]), int(e["c_dst"])
        tr = int(e["transpose"])
        if min(rin, cin, c_src) < 1 or c_dst < c_src or tr not in (0, 1):
            raise ValueError(f"layout entry {i}: bad extents")
        wide = -(-rin // c_src) * c_dst if tr else cin
        drows = cin if tr else rin
        if kp % LAYOUT_TILE or kp < wide or (not tr and c_src != c_dst):
            raise ValueError(f"layout entry {i}: bad row length {kp}")
        src, dst = int(e["src_off"]), int(e["dst_off"])
        if src < 0 or src + rin * cin > blob_elems:
            raise ValueError(f"layout entry {i} reads outside the blob")
        if dst < 0 or dst % 256 or dst + drows * kp * 2 > arena_bytes:
            raise ValueError(f"layout entry {i} writes outside the arena")
        tiles = -(-drows // LAYOUT_TILE) * (kp // LAYOUT_TILE)
        if int(tile_start[i + 1]) - int(tile_start[i]) != tiles:
            raise ValueError(f"layout entry {i}: tile_start is off")
        spans.append((dst, dst + drows * kp * 2))
    spans.sort()
    for (_a0, a1), (b0, _b1) in zip(spans, spans[1:]):
        if b0 < a1:
            raise ValueError("layout entries overlap in the arena")


@dataclass
class Template:
    """Everything a context of one (plan, bucket, dtype) needs besides
    device memory."""
    shapes: List[Tuple[int, ...]]
    root: List[int]                      # alias chains resolved
    bufs: Dict[int, _BufInfo]            # root idx -> workspace slice
    total_bytes: int                     # workspace size
    scratch_off: Dict[int, int]          # op idx -> scratch byte offset
    region_keys: List[tuple]             # in order of first use
    calls: List[tuple]                   # (kind, descs, ints, floats)


def build_template(plan: Plan, batch: int, dtype: str) -> Template:
    e = _Emitter(plan, batch, dtype)
    e.plan_buffers()
    e.emit_calls()
    return Template(e.shapes, e.root, e.bufs, e.total_bytes,
                    e.scratch_off, e.region_keys, e.calls)


class _Emitter:
    def __init__(self, plan: Plan, batch: int, dtype: str):
        self.plan = plan
        self.batch = batch
        self.dtype = dtype
        self.layout = blob_layout(plan)
        self.shapes: List[Tuple[int, ...]] = [
            plan.resolve_shape(t.shape, batch) for t in plan.tensors]
        self.root = [t.alias_of if t.alias_of is not None else t.idx
                     for t in plan.tensors]
        # resolve alias chains
        for i, r in enumerate(self.root):
            seen = 0
            while plan.tensors[r].alias_of is not None and seen < 16:
                r = plan.tensors[r].alias_of
                seen += 1
            self.root[i] = r
        self.region_keys: List[tuple] = []
        self._seen = set()
        self.calls: List[tuple] = []

    # -- buffer planning ---------------------------------------------------
    def _buf_bytes(self, idx: int) -> int:
        esize = 4 if self.plan.tensors[idx].dtype == "i32" else 2
        return max(_numel(self.shapes[idx]) * esize, esize)

    def plan_buffers(self) -> None:
        plan = self.plan
        root = self.root
        live_end: Dict[int, int] = {}
        scratch_sizes: Dict[int, int] = {}   # op_idx -> scratch bytes

        n_ops = len(plan.ops)
        for oi, op in enumerate(plan.ops):
            for i in op.inputs + op.outputs:
                live_end[root[i]] = oi
        for i in plan.sig_outputs.values():
            live_end[root[i]] = n_ops + 1
        for i in plan.sig_inputs.values():
            live_end[root[i]] = max(live_end.get(root[i], -1), 0)

        # scratch sizes (conv channel-pad, gemm K-pad)
        for oi, op in enumerate(plan.ops):
            if op.kind == "gemm":
                a_shape = self.shapes[op.inputs[0]]
                K = a_shape[-1]
                M = int(np.prod(a_shape[:-1]))
                if self.dtype == "fp8":
                    # quantized activations (u8 [M, Kp128]) + row scales
                    Kp = _pad128(K)
                    scratch_sizes[oi] = _pad256b(M * Kp) + M * 4
                elif K % 64 != 0:
                    scratch_sizes[oi] = M * _pad64(K) * 2
            if op.kind == "conv2d":
                R, S, Cin, Kc = op.params["rsck"]
                is_1x1 = (R == 1 and S == 1 and
                          op.params["stride"] == (1, 1) and
                          op.params["pads"] == (0, 0, 0, 0) and
                          Cin % 64 == 0)
                # channel-pad scratch for the C%8!=0 case (RGB stem):
                # input widened to C8 channels, then fused conv
                if not is_1x1 and Cin % 8 != 0:
                    H, W = op.params["hw"]
                    c8 = (Cin + 7) // 8 * 8
                    scratch_sizes[oi] = self.batch * H * W * c8 * 2
            if op.kind in ("conv3d", "conv3d_transpose"):
                # the same channel-pad scratch, over N*D*H*W rows
                Cin = op.params["trsck"][3]
                if Cin % 8 != 0:
                    rows = _numel(self.shapes[op.inputs[0]][:-1])
                    scratch_sizes[oi] = rows * ((Cin + 7) // 8 * 8) * 2
            if op.kind == "lstm":
                scratch_sizes[oi] = self._lstm_scratch(op)[-1]
            if op.kind == "topk_last":
                # a split row's partial results: P lists of k 64-bit
                # composites per row
                rows, cols = _rows_cols(self.shapes[op.inputs[0]])
                P = topk_segments(rows, cols, op.params["k"])
                if P > 1:
                    scratch_sizes[oi] = rows * P * op.params["k"] * 8
            if op.kind == "combined_nms":
                scratch_sizes[oi] = self._nms_scratch(op)[-1]
            if op.kind == "reduce":
                # a split axis's partials: P f32 per output element
                outer, red, inner = self._reduce_view(op)
                P = reduce_segments(outer, red, inner)
                if P > 1:
                    scratch_sizes[oi] = outer * inner * P * 4

        self.bufs: Dict[int, _BufInfo] = {}
        self.scratch_off: Dict[int, int] = {}
        free: List[Tuple[int, int]] = []     # (nbytes, offset)
        cursor = 0

        def alloc(nbytes: int) -> int:
            nonlocal cursor
            nbytes = (nbytes + ALIGN - 1) // ALIGN * ALIGN
            best = None
            for j, (sz, off) in enumerate(free):
                if sz >= nbytes and (best is None or sz < free[best][0]):
                    best = j
            if best is not None:
                sz, off = free.pop(best)
                if sz > nbytes:
                    free.append((sz - nbytes, off + nbytes))
                return off
            off = cursor
            cursor += nbytes
            return off

        def release(off: int, nbytes: int) -> None:
            nbytes = (nbytes + ALIGN - 1) // ALIGN * ALIGN
            free.append((nbytes, off))

        def ensure(idx: int) -> None:
            r = root[idx]
            if r in self.bufs:
                return
            nb = self._buf_bytes(r)
            self.bufs[r] = _BufInfo(alloc(nb), nb, self.shapes[r],
                                    plan.tensors[r].dtype == "i32")

        # inputs first (persistent through the run)
        for i in plan.sig_inputs.values():
            ensure(i)
        for oi, op in enumerate(plan.ops):
            for i in op.outputs:
                ensure(i)
            if oi in scratch_sizes:
                self.scratch_off[oi] = alloc(scratch_sizes[oi])
                release(self.scratch_off[oi], scratch_sizes[oi])
                # NOTE: scratch freed immediately after alloc so the NEXT
                # op's outputs can reuse it; but it must survive through
                # this op — handled because outputs were allocated first.
            for i in op.inputs:
                r = root[i]
                if r in self.bufs and live_end.get(r, -1) == oi and \
                        plan.tensors[r].kind != "input" and \
                        live_end[r] <= n_ops:
                    release(self.bufs[r].offset, self.bufs[r].nbytes)
        self.total_bytes = max(cursor, ALIGN)

    # -- pointer descriptors -----------------------------------------------
    def _weight(self, idx: int):
        """Master copy of weight tensor idx (no alias resolution)."""
        slot = self.layout.slots.get(idx)
        if slot is not None:
            return (("blob",), slot[0] * 2)
        if idx in self.layout.int_idx:
            return (("int", idx), 0)
        raise KeyError(idx)

    def _ptr(self, idx: int):
        r = self.root[idx]
        if self.plan.tensors[r].kind == "weight":
            return self._weight(r)
        return (WS, self.bufs[r].offset)

    def _io(self, op: PlanOp, n_in: int) -> list:
        """The op's first n_in inputs, then its output."""
        return [self._ptr(i) for i in op.inputs[:n_in]] + \
            [self._ptr(op.outputs[0])]

    def _scratch(self, oi: int):
        return (WS, self.scratch_off[oi])

    def _reduce_view(self, op: PlanOp) -> Tuple[int, int, int]:
        """A reduce op's [outer, red, inner] at this batch."""
        view = self.plan.resolve_shape(op.params["view"], self.batch)
        if _numel(view) != _numel(self.shapes[op.inputs[0]]):
            raise RuntimeError(f"GPU reduce: view {view} does not cover "
                               f"input {self.shapes[op.inputs[0]]}")
        return view

    def _weight_shape(self, idx: int) -> Optional[Tuple[int, ...]]:
        """Shape of a constant weight operand, None for an activation."""
        if idx in self.layout.slots or idx in self.layout.int_idx:
            return tuple(self.plan.tensors[idx].weight.shape)
        return None

    def _call(self, kind: str, ptrs: list, ints: list,
              floats: Optional[list] = None) -> None:
        assert kind in KINDS or kind in KINDS_NO_GOLDEN, kind
        for d in ptrs:
            if d is not None and d[0] != WS and d[0] not in self._seen:
                self._seen.add(d[0])
                self.region_keys.append(d[0])
        self.calls.append((kind, ptrs, ints, floats or []))

    # -- call emission -----------------------------------------------------
    def emit_calls(self) -> None:
        call, io = self._call, self._io
        for oi, op in enumerate(self.plan.ops):
            k, p = op.kind, op.params
            xs = self.shapes[op.inputs[0]]
            if k == "eltwise":
                self._c_eltwise(op)
            elif k == "gemm":
                self._c_gemm(op, oi)
            elif k == "conv2d":
                self._c_conv(op, oi)
            elif k == "conv3d":
                self._c_conv3d(op, oi)
            elif k == "conv3d_transpose":
                self._c_conv3d_transpose(op, oi)
            elif k == "lstm":
                self._c_lstm(op, oi)
            elif k == "combined_nms":
                self._c_combined_nms(op, oi)
            elif k == "batched_gemm":
                self._c_bgemm(op)
            elif k == "attention":
                self._c_attention(op)
            elif k == "depthwise_conv":
                n, h, w, c = xs
                ho, wo = p["out_hw"]
                R, S, _C = p["rsc"]
                sh, sw = p["stride"]
                pt, _pb, pl, _pr = p["pads"]
                ints = [n, h, w, c, R, S, sh, sw, pt, pl, ho, wo, _act(p)]
                if p.get("mult", 1) > 1:
                    # optional 14th int, like CONV's 16th `groups`:
                    # c stays the INPUT channel count
                    ints.append(p["mult"])
                if "dilation" in p:
                    # 16-int form [..., act, M, dh, dw]; the planner
                    # admits a dilation with M == 1 only
                    ints += [1, *p["dilation"]]
                call("DEPTHWISE", io(op, 3), ints)
            elif k in _ROWWISE:
                call(_ROWWISE[k], io(op, 1), _rows_cols(xs))
            elif k == "topk_last":
                # ARGMAX_LAST's 4-pointer / 4-int form (argmax is top-1
                # without values): [x, idx, vals, scratch|null],
                # [rows, cols, k, P]
                rows, cols = _rows_cols(xs)
                P = topk_segments(rows, cols, p["k"])
                call("ARGMAX_LAST",
                     [self._ptr(op.inputs[0]), self._ptr(op.outputs[1]),
                      self._ptr(op.outputs[0]),
                      self._scratch(oi) if P > 1 else None],
                     [rows, cols, p["k"], P])
            elif k == "reduce":
                # the reduce forms of MEAN_LAST / MEAN_MID (a mean is one
                # of five functions): [x, y, scratch|null] and
                # [rows, cols, fn, P] or [d0, d1, d2, fn, P]
                outer, red, inner = self._reduce_view(op)
                P = reduce_segments(outer, red, inner)
                ptrs = io(op, 1) + [self._scratch(oi) if P > 1 else None]
                fn = _REDUCE_CODE[p["fn"]]
                if inner == 1:
                    call("MEAN_LAST", ptrs, [outer, red, fn, P])
                else:
                    call("MEAN_MID", ptrs, [outer, red, inner, fn, P])
            elif k == "layernorm":
                call("LAYERNORM", io(op, 3), _rows_cols(xs),
                     [float(p["eps"])])
            elif k == "bn_act":
                c = xs[-1]
                call("BN_ACT", io(op, 3),
                     [int(np.prod(xs)) // c, c, _act(p)])
            elif k == "global_mean":
                n, h, w, c = xs
                call("MEAN_MID", io(op, 1), [n, h * w, c])
            elif k == "reduce_mean_mid":
                d0, d1, d2 = xs
                call("MEAN_MID", io(op, 1), [d0, d1, d2])
            elif k == "pool":
                n, h, w, c = xs
                ho, wo = p["out_hw"]
                kh, kw = p["ksize"]
                sh, sw = p["stride"]
                pt, pb, pl, pr = p["pads"]
                call("POOL", io(op, 1),
                     [1 if p["mode"] == "max" else 0,
                      n, h, w, c, ho, wo, kh, kw, sh, sw, pt, pl])
            elif k == "pool3d":
                # POOL's 18-int form
                n, d, h, w, c = xs
                do, ho, wo = p["out_dhw"]
                pf, _pk, pt, _pb, pl, _pr = p["pads"]
                call("POOL", io(op, 1),
                     [1 if p["mode"] == "max" else 0, n, d, h, w, c,
                      do, ho, wo, *p["ksize"], *p["stride"], pf, pt, pl])
            elif k == "resize":
                n, h, w, c = xs
                ho, wo = p["out_hw"]
                if (h, w) != tuple(p["in_hw"]) or \
                        p["mode"] not in ("nearest", "bilinear"):
                    raise RuntimeError(f"GPU resize: bad params {p}")
                call("RESIZE", io(op, 1),
                     [n, h, w, c, ho, wo,
                      1 if p["mode"] == "bilinear" else 0,
                      1 if p["align_corners"] else 0,
                      1 if p["half_pixel_centers"] else 0])
            elif k == "zero_insert":
                n, h, w, c = xs
                sh, sw = p["stride"]
                if tuple(self.shapes[op.outputs[0]]) != \
                        (n, (h - 1) * sh + 1, (w - 1) * sw + 1, c):
                    raise RuntimeError(f"GPU zero_insert: bad params {p}")
                call("ZERO_INSERT", io(op, 1), [n, h, w, c, sh, sw])
            elif k == "transpose":
                out_shape = self.shapes[op.outputs[0]]
                in_strides = _strides(xs)
                call("TRANSPOSE", io(op, 1),
                     [len(out_shape)] + list(out_shape) +
                     [in_strides[q] for q in p["perm"]] +
                     [int(np.prod(out_shape))])
            elif k == "gather":
                ishape = self.shapes[op.inputs[1]]
                call("GATHER", io(op, 2),
                     [_numel(ishape), int(np.prod(xs[1:]))])
            elif k == "strided_copy":
                out_shape = self.shapes[op.outputs[0]]
                istr = _strides(xs)
                starts, steps = p["starts"], p["steps"]
                shrink = p["shrink"]
                offset = sum(starts[d] * istr[d] for d in range(len(xs)))
                strides_out = [istr[d] * steps[d] for d in range(len(xs))
                               if not shrink[d]]
                src, dst = io(op, 1)
                call("TRANSPOSE", [_off(src, offset * 2), dst],
                     [max(len(out_shape), 1)] + (list(out_shape) or [1]) +
                     (strides_out or [1]) + [_numel(out_shape)])
            elif k == "cast":
                call("CAST", io(op, 1),
                     [_numel(xs), 0 if p["mode"] == "i2f" else 1])
            elif k == "concat":
                out_shape = self.shapes[op.outputs[0]]
                axis = p["axis"]
                ostr = _strides(out_shape)
                off_elems = 0
                for inp in op.inputs:
                    ish = self.shapes[inp]
                    call("SCATTER",
                         [self._ptr(inp),
                          _off(self._ptr(op.outputs[0]), off_elems * 2)],
                         [len(ish)] + list(ish) + ostr + [_numel(ish)])
                    off_elems += ish[axis] * ostr[axis]
            elif k == "pad":
                pads = p["pads"]
                if len(xs) != 4 or any(p_[0] or p_[1]
                                       for p_ in (pads[0], pads[3])):
                    raise RuntimeError("GPU pad: only NHWC H/W pads")
                call("PAD_NHWC", io(op, 1),
                     list(xs) + [pads[1][0], pads[1][1], pads[2][0],
                                 pads[2][1]])
            else:
                raise RuntimeError(f"GPU lowering: unsupported op {k}")

    def _c_attention(self, op: PlanOp) -> None:
        p = op.params
        b_, s_, h_, d_ = self.shapes[op.inputs[0]]
        ptrs = self._io(op, 3)
        ints = [b_, s_, h_, d_]
        if len(op.inputs) > 3:
            # additive bias [b,h,q,S] (rank-4 padded), element strides
            # with 0 = broadcast; checked against the resolved shape so
            # a stride never walks past it
            bshape = tuple(self.shapes[op.inputs[3]])
            bshape = (1,) * (4 - len(bshape)) + bshape
            batched, bh, bq = p["bias_dims"]
            want = (b_ if batched else 1, bh, bq, s_)
            if bshape != want or bh not in (1, h_) or bq not in (1, s_):
                raise ValueError(
                    f"attention bias shape {bshape} does not "
                    f"match plan {want}")
            ptrs.append(self._ptr(op.inputs[3]))
            ints += [bh * bq * s_ if batched else 0,
                     bq * s_ if bh == h_ else 0,
                     s_ if bq == s_ else 0]
        self._call("ATTENTION", ptrs, ints, [float(p["scale"])])

    def _bcast_ints(self, out_shape, a_shape, b_shape):
        nd = len(out_shape)
        if nd > 6:
            raise RuntimeError("eltwise rank > 6")

        def strides_for(shape):
            shape = list(shape)
            shape = [1] * (nd - len(shape)) + shape
            st = [0] * nd
            acc = 1
            for d in range(nd - 1, -1, -1):
                if shape[d] == out_shape[d] and shape[d] != 1:
                    st[d] = acc
                elif shape[d] == 1 and out_shape[d] != 1:
                    st[d] = 0
                elif shape[d] == out_shape[d]:
                    st[d] = acc   # both 1
                else:
                    raise RuntimeError(
                        f"cannot broadcast {shape} to {out_shape}")
                acc *= shape[d]
            return st

        return strides_for(a_shape), strides_for(b_shape)

    def _c_eltwise(self, op: PlanOp) -> None:
        fn = _ELT_CODE[op.params["fn"]]
        out_shape = self.shapes[op.outputs[0]]
        n_out = _numel(out_shape)
        if len(op.inputs) == 1:
            self._call("ELT_UNARY", self._io(op, 1), [n_out, fn])
            return
        a, b = op.inputs
        sa_shape, sb_shape = self.shapes[a], self.shapes[b]
        if tuple(sa_shape) == tuple(out_shape) == tuple(sb_shape):
            ints = [n_out, fn, 1, n_out, 1, 1]
        else:
            sa, sb = self._bcast_ints(out_shape, sa_shape, sb_shape)
            ints = [n_out, fn, len(out_shape)] + list(out_shape) + sa + sb
        self._call("ELT_BINARY", self._io(op, 2), ints)

    def _c_gemm(self, op: PlanOp, oi: int) -> None:
        p = op.params
        a_shape = self.shapes[op.inputs[0]]
        M = int(np.prod(a_shape[:-1]))
        K = a_shape[-1]
        if p.get("trans_a"):
            raise RuntimeError("gemm trans_a unsupported on GPU")
        fp8 = self.dtype == "fp8"
        wshape = self._weight_shape(op.inputs[1])
        if wshape is None:
            raise RuntimeError(
                "fp8 gemm requires a constant weight" if fp8 else
                "GPU gemm requires a constant weight operand; "
                "activation x activation MatMul must be BatchMatMul")
        # the kernels read the weight pre-transposed to [N][Kp] (the
        # graph holds [K,N] unless trans_b), K zero-padded
        N, Kw = wshape if p.get("trans_b") else wshape[::-1]
        Kp = _pad128(Kw) if fp8 else _pad64(Kw)
        wkey = (op.inputs[1], bool(p.get("trans_b")))
        ni = 2
        bias = res = None
        if p.get("has_bias"):
            bias = self._weight(op.inputs[ni])
            ni += 1
        if p.get("residual"):
            res = self._ptr(op.inputs[ni])
        a_ptr, out = self._io(op, 1)
        ints = [M, N, Kp, _act(p)]
        if fp8:
            # fp8 serving path: rowwise-quantize the activation into
            # scratch, then the e4m3 MFMA GEMM with per-row x per-col
            # dequant in the epilogue (engine.dtype: fp8)
            q_ptr = self._scratch(oi)
            sa_ptr = _off(q_ptr, _pad256b(M * Kp))
            self._call("QUANT_FP8", [a_ptr, q_ptr, sa_ptr], [M, K, Kp])
            self._call("GEMM_FP8",
                       [q_ptr, sa_ptr, (("f8q",) + wkey, 0),
                        (("f8s",) + wkey, 0), bias, res, out], ints)
            return
        if Kp != K:
            # zero-pad the activation's K to the weight's 64-aligned Kp
            scratch = self._scratch(oi)
            self._call("PAD_LAST", [a_ptr, scratch], [M, K, Kp])
            a_ptr = scratch
        self._call("GEMM", [a_ptr, (("gw",) + wkey, 0), bias, res, out],
                   ints, [1.0])

    def _c_conv(self, op: PlanOp, oi: int) -> None:
        p = op.params
        R, S, Cin, Kc = p["rsck"]
        sh, sw = p["stride"]
        pt, pb, pl, pr = p["pads"]
        Ho, Wo = p["out_hw"]
        x = op.inputs[0]
        w_idx = op.inputs[1]
        n, H, W, C = self.shapes[x]
        M = n * Ho * Wo
        bias = self._weight(op.inputs[2])
        res = self._ptr(op.inputs[3]) if p.get("residual") else None
        wshape = self._weight_shape(w_idx)            # [R,S,C,K] master
        if wshape is None:
            raise KeyError(f"no master weight for tensor {w_idx}")
        wR, wS, wC, _wK = wshape
        act = _act(p)
        out = self._ptr(op.outputs[0])
        zeros = (("zeros",), 0)
        groups = p.get("groups", 1)
        if "dilation" in p:
            # dilated implicit-GEMM: the 18-int form [..., act, groups,
            # dh, dw] with groups written as 1 (the planner rejects a
            # dilated grouped conv and C % 8 != 0). Never the 1x1 GEMM
            # shortcut or the channel widening.
            self._call("CONV",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res,
                        zeros, out],
                       [n, H, W, C, Kc, R, S, sh, sw, pt, pl, Ho, Wo,
                        _pad64(wR * wS * wC), act, 1, *p["dilation"]])
        elif groups > 1:
            # grouped implicit-GEMM: the master is [R,S,Cg,K] (Cg % 8 ==
            # 0 by the planner's merge rule), C the input's full channel
            # count; groups rides as an optional 16th int. Never the
            # 1x1 GEMM shortcut or the channel widening.
            self._call("CONV",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res,
                        zeros, out],
                       [n, H, W, C, Kc, R, S, sh, sw, pt, pl, Ho, Wo,
                        _pad64(wR * wS * wC), act, groups])
        elif R == 1 and S == 1 and (sh, sw) == (1, 1) and \
                (pt, pb, pl, pr) == (0, 0, 0, 0) and C % 64 == 0:
            self._call("GEMM",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res, out],
                       [M, Kc, C, act], [1.0])
        elif C % 8 == 0:
            # fused implicit-GEMM (no im2col materialization)
            self._call("CONV",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res,
                        zeros, out],
                       [n, H, W, C, Kc, R, S, sh, sw, pt, pl, Ho, Wo,
                        _pad64(wR * wS * wC), act])
        else:
            # C % 8 != 0 (RGB stem): widen channels to C8 with zeros,
            # then the fused conv with channel-padded weights
            c8 = (C + 7) // 8 * 8
            scratch = self._scratch(oi)
            self._call("PAD_LAST", [self._ptr(x), scratch],
                       [n * H * W, C, c8])
            self._call("CONV",
                       [scratch, (("cw", w_idx, "cpad", c8), 0), bias,
                        res, zeros, out],
                       [n, H, W, c8, Kc, R, S, sh, sw, pt, pl, Ho, Wo,
                        _pad64(wR * wS * c8), act])

    def _c_conv3d(self, op: PlanOp, oi: int) -> None:
        """CONV's 23-int form: the 15 ints of a 2-D conv on the (H, W)
        axes, groups / dh / dw written as 1, then [D, T, sd, pf, Do]. The
        master weight is [T*R,S,C,K], so ("cw", idx) is
        [Kc][pad64(T*R*S*C)] in (t,r,s,c) order. The 1x1x1 GEMM shortcut
        and the C % 8 != 0 channel widening are the 2-D ones over
        N*D*H*W rows."""
        p = op.params
        T, R, S, C, Kc = p["trsck"]
        sd, sh, sw = p["stride"]
        pf, pk, pt, pb, pl, pr = p["pads"]
        Do, Ho, Wo = p["out_dhw"]
        x, w_idx = op.inputs[0], op.inputs[1]
        n, D, H, W, xC = self.shapes[x]
        if self._weight_shape(w_idx) != (T * R, S, C, Kc) or xC != C:
            raise KeyError(f"no [T*R,S,C,K] master weight for tensor {w_idx}")
        bias = self._weight(op.inputs[2])
        res = self._ptr(op.inputs[3]) if p.get("residual") else None
        act = _act(p)
        out = self._ptr(op.outputs[0])
        zeros = (("zeros",), 0)

        def ints(c):
            return [n, H, W, c, Kc, R, S, sh, sw, pt, pl, Ho, Wo,
                    _pad64(T * R * S * c), act, 1, 1, 1, D, T, sd, pf, Do]

        if (T, R, S) == (1, 1, 1) and (sd, sh, sw) == (1, 1, 1) and \
                not any(p["pads"]) and C % 64 == 0:
            self._call("GEMM",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res, out],
                       [n * D * H * W, Kc, C, act], [1.0])
        elif C % 8 == 0:
            self._call("CONV",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res, zeros,
                        out], ints(C))
        else:
            c8 = (C + 7) // 8 * 8
            scratch = self._scratch(oi)
            self._call("PAD_LAST", [self._ptr(x), scratch],
                       [n * D * H * W, C, c8])
            self._call("CONV",
                       [scratch, (("cw", w_idx, "cpad", c8), 0), bias, res,
                        zeros, out], ints(c8))

    def _c_conv3d_transpose(self, op: PlanOp, oi: int) -> None:
        """CONV's 24-int form: the 23-int form's slots with x's extents in
        N,D,H,W,C, y's in Do,Ho,Wo,Kc, the full filter in T,R,S, the low
        pads of the forward conv in pf,pt,pl, and a 24th int 1,
        "transposed". The master weight is [n_taps,1,Ci,Co] in the kernel's
        phase-major tap order (planner.conv3d_transpose_phases), so
        ("cw", idx) is [Kc][pad64(n_taps*C)]; C % 8 != 0 is widened as in
        _c_conv3d."""
        p = op.params
        T, R, S, C, Kc = p["trsck"]
        sd, sh, sw = p["stride"]
        pf, pt, pl = p["pads"]
        Do, Ho, Wo = p["out_dhw"]
        x, w_idx = op.inputs[0], op.inputs[1]
        n, D, H, W, xC = self.shapes[x]
        c8 = (C + 7) // 8 * 8
        n_taps = conv3d_transpose_taps((T, R, S), (sd, sh, sw), c8)
        if self._weight_shape(w_idx) != (n_taps, 1, C, Kc) or xC != C:
            raise KeyError(f"no [n_taps,1,Ci,Co] master weight for tensor "
                           f"{w_idx}")
        bias = self._weight(op.inputs[2])
        res = self._ptr(op.inputs[3]) if p.get("residual") else None
        out = self._ptr(op.outputs[0])
        zeros = (("zeros",), 0)
        ints = [n, H, W, c8, Kc, R, S, sh, sw, pt, pl, Ho, Wo,
                _pad64(n_taps * c8), _act(p), 1, 1, 1, D, T, sd, pf, Do, 1]
        if C % 8 == 0:
            self._call("CONV",
                       [self._ptr(x), (("cw", w_idx), 0), bias, res, zeros,
                        out], ints)
        else:
            scratch = self._scratch(oi)
            self._call("PAD_LAST", [self._ptr(x), scratch],
                       [n * D * H * W, C, c8])
            self._call("CONV",
                       [scratch, (("cw", w_idx, "cpad", c8), 0), bias, res,
                        zeros, out], ints)

    def _lstm_scratch(self, op: PlanOp) -> Tuple[int, int, int]:
        """Byte offsets of (cstate, padded x) inside an lstm op's scratch,
        and its size. pre [T*B, N] bf16 sits at 0, then the f32 cell
        state [B, H]; when I % 64 != 0 the K-padded copy of x the GEMM
        reads comes last."""
        p = op.params
        rows = _numel(self.shapes[op.inputs[0]][:-1])
        c_off = _pad256b(rows * lstm_cols(p["H"]) * 2)
        x_off = c_off + _pad256b(rows // p["T"] * p["H"] * 4)
        pad = rows * _pad64(p["I"]) * 2 if p["I"] % 64 else 0
        return c_off, x_off, x_off + pad

    def _c_lstm(self, op: PlanOp, oi: int) -> None:
        """GEMM (x W_x + b for all T*B rows, into scratch `pre`) then one
        LSTM call. ptrs: [pre, W_h, wci|null, wcf|null, wco|null, h0|null,
        c0|null, cstate, h, cs|null]; ints: [T, B, H, st_t, st_b, pre_t,
        pre_b], st_* the element strides of row (t, b) of h and cs, pre_*
        the row strides of pre (its rows follow x's, so a batch-major x
        gives pre_t = 1, pre_b = T); floats: [cell_clip]. The projection
        is the bf16 GEMM under every engine dtype."""
        p = op.params
        T, I, H = p["T"], p["I"], p["H"]
        N = lstm_cols(H)
        x, wx, wh, b = op.inputs[:4]
        rows = _numel(self.shapes[x][:-1])
        Bn = rows // T
        if self._weight_shape(wx) != (I, N) or \
                self._weight_shape(wh) != (H, N) or \
                self.shapes[x][-1] != I or rows != T * Bn:
            raise KeyError(f"lstm: weights do not match x {self.shapes[x]}")
        ni = 4
        peep = [None, None, None]
        if p["peephole"]:
            peep = [self._weight(i) for i in op.inputs[4:7]]
            ni = 7
        h0 = c0 = None
        if p["h0"]:
            h0 = self._ptr(op.inputs[ni])
            ni += 1
        if p["c0"]:
            c0 = self._ptr(op.inputs[ni])
        pre = self._scratch(oi)
        c_off, x_off, _ = self._lstm_scratch(op)
        a_ptr = self._ptr(x)
        if I % 64:
            self._call("PAD_LAST", [a_ptr, _off(pre, x_off)],
                       [rows, I, _pad64(I)])
            a_ptr = _off(pre, x_off)
        self._call("GEMM", [a_ptr, (("gw", wx, False), 0), self._weight(b),
                            None, pre], [rows, N, _pad64(I), 0], [1.0])
        st = [H, T * H] if p["h_batch_major"] else [Bn * H, H]
        pst = [1, T] if p["x_batch_major"] else [Bn, 1]
        cs = self._ptr(op.outputs[1]) if p["cs"] else None
        self._call("LSTM",
                   [pre, (("gw", wh, False), 0), *peep, h0, c0,
                    _off(pre, c_off), self._ptr(op.outputs[0]), cs],
                   [T, Bn, H, *st, *pst], [float(p["cell_clip"])])

    def _nms_scratch(self, op: PlanOp) -> Tuple[int, ...]:
        """Byte offsets of (cls_score, cls_idx, slot, val, top-k partials)
        inside a combined_nms op's scratch, and its size. The class-major
        scores [B,C,N] bf16 sit at 0 (nothing when C == 1); cls_score bf16
        and cls_idx i32 are [B, C*P]; slot i32 and val bf16 are the top-k
        result [B, k]; the partials are topk_last's."""
        p = op.params
        nb = self.shapes[op.inputs[1]][0]
        slots = p["c"] * p["per_class"]
        k = min(p["max_total"], slots)
        seg = topk_segments(nb, slots, k)
        sizes = [nb * p["c"] * p["n"] * 2 if p["c"] > 1 else 0,
                 nb * slots * 2, nb * slots * 4, nb * k * 4, nb * k * 2,
                 nb * seg * k * 8 if seg > 1 else 0]
        offs = [0]
        for sz in sizes:
            offs.append(offs[-1] + _pad256b(sz))
        return tuple(offs[1:])

    def _c_combined_nms(self, op: PlanOp, oi: int) -> None:
        """TRANSPOSE (scores to class-major, skipped when C == 1), NMS
        select, ARGMAX_LAST's top-k form over the C*P per-class slots, NMS
        gather. Select, ptrs: [scores_cm, boxes, cls_score, cls_idx]; ints:
        [B, N, C, q, P]; floats: [iou_thr, score_thr]. Gather, ptrs: [slot,
        val, cls_idx, boxes, out_boxes, out_scores, out_classes, out_valid];
        ints: [B, N, C, q, P, k, M, clip]."""
        p = op.params
        n, c, q, P, M = p["n"], p["c"], p["q"], p["per_class"], p["max_total"]
        nb = self.shapes[op.inputs[1]][0]
        if tuple(self.shapes[op.inputs[0]]) != (nb, n, q, 4) or \
                tuple(self.shapes[op.inputs[1]]) != (nb, n, c):
            raise RuntimeError(f"GPU combined_nms: bad params {p}")
        boxes, scores = (self._ptr(i) for i in op.inputs)
        base = self._scratch(oi)
        o_score, o_idx, o_slot, o_val, o_part, _ = self._nms_scratch(op)
        cls_score, cls_idx = _off(base, o_score), _off(base, o_idx)
        slot, val = _off(base, o_slot), _off(base, o_val)
        if c > 1:
            self._call("TRANSPOSE", [scores, base],
                       [3, nb, c, n, n * c, 1, c, nb * c * n])
            scores = base
        self._call("NMS", [scores, boxes, cls_score, cls_idx],
                   [nb, n, c, q, P],
                   [float(p["iou_thr"]), float(p["score_thr"])])
        k = min(M, c * P)
        seg = topk_segments(nb, c * P, k)
        self._call("ARGMAX_LAST",
                   [cls_score, slot, val,
                    _off(base, o_part) if seg > 1 else None],
                   [nb, c * P, k, seg])
        self._call("NMS",
                   [slot, val, cls_idx, boxes] +
                   [self._ptr(o) for o in op.outputs],
                   [nb, n, c, q, P, k, M, 1 if p["clip"] else 0])

    def _c_bgemm(self, op: PlanOp) -> None:
        p = op.params
        a_shape = self.shapes[op.inputs[0]]
        b_shape = self.shapes[op.inputs[1]]
        if p.get("trans_a"):
            raise RuntimeError("batched_gemm trans_a unsupported")
        trans_b = bool(p.get("trans_b"))
        M, K = a_shape[-2], a_shape[-1]
        N = b_shape[-2] if trans_b else b_shape[-1]
        bat_a = int(np.prod(a_shape[:-2])) if len(a_shape) > 2 else 1
        bat_b = int(np.prod(b_shape[:-2])) if len(b_shape) > 2 else 1
        sA = M * K if bat_a > 1 else 0
        sB = (b_shape[-1] * b_shape[-2]) if bat_b > 1 else 0
        self._call("BGEMM", self._io(op, 2),
                   [max(bat_a, bat_b), M, N, K, sA, sB, M * N,
                    1 if trans_b else 0], [1.0])

"""The compact master blob (emit.live_blob_layout) and the one-call
repeat load (ext.restore_weights, csrc/ops/weight_layout.hip).

Call emission addresses the blob by emit.blob_layout, which gives a slot
to every float weight of the plan, the ones the planner folded away
included. The device blob, its pinned host copy and the layout table use
live_blob_layout: the same slots in the same order without the dead ones.
The CPU tests hold the two against each other on every fixture builder;
the GPU tests run the native restore call on a hand-made plan and through
the pool / loader path of the headline bench.

Tolerances of the loader test are those of the tests it extends:
rtol 0.05, atol 0.02 against the first load
(test_weight_layout.test_repeat_load_restores_through_the_kernel) and
against the CPU fp32 reference
(test_gpu_serving.test_template_capture_only_numerics); two repeat loads
run the same captured kernels over the same bytes and must agree bit for
bit.
"""
import functools
import os
import shutil
from bisect import bisect_right

import numpy as np
import pytest
import torch

from test_weight_layout import (HAND_MADE, _compile, interpret, make_blob,
                                ref_region)
from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.planner import Plan, PlanOp, PlanTensor
from tfservingcache_amd.models import builders

FIXTURES = {
    "resnet": (builders.build_resnet50, dict(image_size=32, num_classes=10)),
    "bert": (builders.build_bert, dict(seq_len=16, hidden=64, layers=1,
                                       heads=2)),
    "mobilenet": (builders.build_mobilenet_v2,
                  dict(image_size=32, num_classes=10, width_mult=0.25)),
    "lstm": (builders.build_lstm_tagger, {}),
    "ssd": (builders.build_ssd_detector, {}),
    "unet": (builders.build_unet, {}),
    "resnext": (builders.build_resnext, {}),
}
REGION_KINDS = ("gw", "cw", "f8q", "f8s")


@functools.lru_cache(maxsize=None)
def _plan(name):
    builder, kw = FIXTURES[name]
    return _compile(builder, **kw)


def _blob_ptrs(tmpl):
    """Byte offsets of every ("blob",) pointer of a template."""
    return [d[1] for _kind, descs, _i, _f in tmpl.calls for d in descs
            if d is not None and d[0] == ("blob",)]


def _full_slot_of(full, byte_off):
    """(idx, slot start, n) of the full-layout slot holding byte_off."""
    order = sorted((off, n, idx) for idx, (off, n) in full.slots.items())
    i = bisect_right([o for o, _n, _i in order], byte_off // 2) - 1
    off, n, idx = order[i]
    assert off * 2 <= byte_off < (off + emit._pad128(n)) * 2
    return idx, off, n


def make_compact_blob(plan):
    """bf16 compact blob of a plan on the CPU (slot padding zero), as
    test_weight_layout.make_blob makes the full one."""
    layout = emit.live_blob_layout(plan)
    blob = torch.zeros(layout.total, dtype=torch.bfloat16)
    for idx, (off, n) in layout.slots.items():
        w = np.array(plan.tensors[idx].weight, dtype=np.float32)
        blob[off:off + n] = torch.from_numpy(w).view(-1)
    return layout, blob


def _u8(t):
    return t.contiguous().view(torch.uint8).numpy()


# -- CPU -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_templates_refer_to_live_slots_only(name):
    plan = _plan(name)
    full, live = emit.blob_layout(plan), emit.live_blob_layout(plan)
    assert set(live.slots) <= set(full.slots)
    assert live.int_idx == full.int_idx and live.full_total == full.total
    # same order, same padding
    assert [i for i in full.slots if i in live.slots] == list(live.slots)
    assert live.total == sum(emit._pad128(n) for _o, n in live.slots.values())
    emitted = 0
    for dtype in ("bf16", "fp8"):
        for bucket in (1, 2, 8):
            tmpl = emit.build_template(plan, bucket, dtype)
            emitted += 1
            for off in _blob_ptrs(tmpl):
                idx, _o, _n = _full_slot_of(full, off)
                assert idx in live.slots, (dtype, bucket, off, idx)
            for key in tmpl.region_keys:
                if key[0] in REGION_KINDS:
                    assert key[1] in live.slots, (dtype, bucket, key)
    assert emitted == 6


def test_what_the_compaction_saves():
    full, live = (f(_plan("resnet")) for f in (emit.blob_layout,
                                               emit.live_blob_layout))
    assert round(full.total * 2 / 1e6, 2) == 94.13
    assert round(live.total * 2 / 1e6, 2) == 47.01
    full, live = (f(_plan("bert")) for f in (emit.blob_layout,
                                             emit.live_blob_layout))
    assert full.total * 0.99 < live.total <= full.total


def _dead_ends_plan():
    """Five float weights; the first and the last are in no op's inputs,
    the third is live only as the root of an alias."""
    rng = np.random.default_rng(3)
    shapes = [(5, 33), (70, 130), (9,), (3, 3, 8, 1), (257,)]
    tensors = [PlanTensor(i, s, "f32", "weight",
                          weight=rng.standard_normal(s).astype(np.float32))
               for i, s in enumerate(shapes)]
    tensors.append(PlanTensor(5, (3, 3), "f32", "weight", alias_of=2))
    ops = [PlanOp("noop", [1, 5], []), PlanOp("noop", [3], [])]
    return Plan(tensors, ops, {}, {}, {})


def _assert_remap_keeps_bytes(plan, ptrs):
    full, fblob = make_blob(plan)
    live, cblob = make_compact_blob(plan)
    fb, cb = _u8(fblob), _u8(cblob)
    for off in ptrs:
        _idx, start, n = _full_slot_of(full, off)
        to_end = (start + n) * 2 - off
        assert to_end > 0
        c = live.compact_byte_offset(off)
        assert c % 2 == off % 2 and c + to_end <= live.total * 2
        assert np.array_equal(cb[c:c + to_end], fb[off:off + to_end]), off


@pytest.mark.parametrize("name", ["resnet", "bert", "lstm"])
def test_remapped_pointers_read_the_same_bytes(name):
    plan = _plan(name)
    full = emit.blob_layout(plan)
    ptrs = set()
    for dtype in ("bf16", "fp8"):
        ptrs.update(_blob_ptrs(emit.build_template(plan, 2, dtype)))
    assert ptrs
    # a hand-made pointer into the middle of the last slot a kernel reads
    _idx, start, n = _full_slot_of(full, max(ptrs))
    assert n > 2
    ptrs.add((start + n // 2) * 2)
    _assert_remap_keeps_bytes(plan, sorted(ptrs))


def test_remap_with_dead_first_and_last_tensor():
    plan = _dead_ends_plan()
    full, live = emit.blob_layout(plan), emit.live_blob_layout(plan)
    assert list(full.slots) == [0, 1, 2, 3, 4]
    assert list(live.slots) == [1, 2, 3]
    assert live.slots[1][0] == 0 and live.full_starts[0] == full.slots[1][0]
    ptrs = [full.slots[i][0] * 2 for i in (1, 2, 3)]
    ptrs.append((full.slots[1][0] + 4567) * 2)        # mid-slot
    _assert_remap_keeps_bytes(plan, ptrs)
    # the padding of a live slot still maps; a dead slot does not
    live.compact_byte_offset((full.slots[2][0] + 100) * 2)
    for dead in (0, 4):
        with pytest.raises(KeyError):
            live.compact_byte_offset(full.slots[dead][0] * 2)
    with pytest.raises(KeyError):
        live.compact_byte_offset(full.total * 2)


def _arena_entries(plan, keys):
    """Regions in `keys` order at _pad256b offsets, sized from shapes."""
    entries, off = [], 0
    for key in keys:
        ent = emit._layout_entry(plan, key)
        nb = ent[7] * ent[6] * 2
        entries.append((key, off, nb, torch.bfloat16, (ent[7], ent[6])))
        off = emit._pad256b(off + nb)
    return entries, off


@pytest.mark.parametrize("name", ["resnet", "bert"])
def test_compact_table_writes_the_same_arena(name):
    plan = _plan(name)
    keys = [k for k in emit.build_template(plan, 2, "bf16").region_keys
            if k[0] in ("gw", "cw")]
    if name == "resnet":
        assert any(len(k) == 4 and k[2] == "cpad" for k in keys)
    entries, size = _arena_entries(plan, keys)
    full, fblob = make_blob(plan)
    live, cblob = make_compact_blob(plan)
    t_full, ts_full, cov_full = emit.weight_layout_table(plan, entries)
    t_live, ts_live, cov_live = emit.weight_layout_table(plan, entries,
                                                         layout=live)
    assert cov_full == cov_live == set(keys)
    assert np.array_equal(ts_full, ts_live)
    same = [f for f in emit.LAYOUT_ENTRY_DTYPE.names if f != "src_off"]
    assert np.array_equal(t_full[same], t_live[same])
    assert (t_live["src_off"] <= t_full["src_off"]).all()
    emit.check_layout_table(t_live, ts_live, live.total, size)
    a_full = np.full(size, 0xFF, np.uint8)
    a_live = np.full(size, 0xFF, np.uint8)
    interpret(t_full, _u8(fblob).view(np.uint16), a_full)
    interpret(t_live, _u8(cblob).view(np.uint16), a_live)
    assert np.array_equal(a_full, a_live)


def test_check_refuses_a_table_that_reads_past_the_compact_blob():
    plan = _plan("resnet")
    keys = [k for k in emit.build_template(plan, 2, "bf16").region_keys
            if k[0] in ("gw", "cw")]
    entries, size = _arena_entries(plan, keys)
    live = emit.live_blob_layout(plan)
    t_live, ts, _ = emit.weight_layout_table(plan, entries, layout=live)
    emit.check_layout_table(t_live, ts, live.total, size)
    last = int((t_live["src_off"] + t_live["rin"].astype(np.int64)
                * t_live["cin"]).max())
    with pytest.raises(ValueError):
        emit.check_layout_table(t_live, ts, last - 1, size)
    # a table in full coordinates over the compact blob
    t_full, ts_full, _ = emit.weight_layout_table(plan, entries)
    with pytest.raises(ValueError):
        emit.check_layout_table(t_full, ts_full, live.total, size)


# -- GPU: the native call on a hand-made plan ------------------------------
def _hand_made_case():
    """The HAND_MADE regions of test_weight_layout over a plan that also
    has a dead tensor between two live ones, a vector kernels read in
    place and an int weight (a pinned span of the arena)."""
    rng = np.random.default_rng(11)
    tensors, keys, seen = [], [], {}

    def add(shape, dtype="f32"):
        w = rng.standard_normal(shape).astype(np.float32) if dtype == "f32" \
            else rng.integers(-9, 9, shape).astype(np.int32)
        tensors.append(PlanTensor(len(tensors), shape, dtype, "weight",
                                  weight=w))
        return len(tensors) - 1

    dead = []
    for n, (kind, shape, extra) in enumerate(HAND_MADE):
        idx = seen.get(shape)
        if idx is None:
            idx = seen[shape] = add(shape)
            if n == 0:
                dead.append(add((5, 33)))       # dead, between two live
        keys.append(("gw", idx, extra) if kind == "gw" else
                    ("cw", idx) if kind == "cw" else
                    ("cw", idx, "cpad", extra))
    vec = add((64,))
    int_idx = add((37,), "i32")
    dead.append(add((300,)))                    # dead, last
    live_in = [t.idx for t in tensors if t.idx not in dead]
    plan = Plan(tensors, [PlanOp("noop", live_in, [])], {}, {}, {})
    return plan, keys, vec, int_idx, dead


class _Restore:
    """Host and device buffers of one restore_weights call."""

    def __init__(self):
        from tfservingcache_amd.engine.gpu import _load_backend
        _t, self.ext = _load_backend()
        self.dev = "cuda:0"
        plan, keys, self.vec, int_idx, dead = _hand_made_case()
        self.plan = plan
        self.live, cblob = make_compact_blob(plan)
        assert not set(dead) & set(self.live.slots)
        assert self.live.total < emit.blob_layout(plan).total
        self.cblob = cblob
        # arena: the bf16 regions with the int region in their middle
        bf, off = [], 0
        ints = torch.from_numpy(plan.tensors[int_idx].weight.copy())
        self.entries, self.want_regions = [], []
        for n, key in enumerate(keys):
            o, cnt = self.live.slots[key[1]]
            r = ref_region(cblob[o:o + cnt].view(
                tuple(plan.tensors[key[1]].weight.shape)), key)
            self.entries.append((key, off, r.numel() * 2, torch.bfloat16,
                                 tuple(r.shape)))
            self.want_regions.append(_u8(r).ravel())
            off = emit._pad256b(off + r.numel() * 2)
            if n == 2:
                self.int_entry = (("int", int_idx), off, ints.numel() * 4,
                                  torch.int32, tuple(ints.shape))
                off = emit._pad256b(off + ints.numel() * 4)
        self.size = off
        self.table, self.tile_start, covered = emit.weight_layout_table(
            plan, self.entries, layout=self.live)
        assert covered == set(keys)
        emit.check_layout_table(self.table, self.tile_start,
                                self.live.total, self.size)
        # pinned: the compact blob and the remainder (the int bytes,
        # behind 256 bytes that belong to no span)
        self.blob_pin = cblob.pin_memory()
        self.rem_pin = torch.full((1024,), 0x5A, dtype=torch.uint8).pin_memory()
        nb = self.int_entry[2]
        self.rem_pin[256:256 + nb] = torch.from_numpy(_u8(ints).ravel().copy())
        self.spans = [(self.int_entry[1], 256, nb)]
        self.want = np.full(self.size, 0xFF, np.uint8)
        for (_k, o, n_, _d, _s), r in zip(self.entries, self.want_regions):
            self.want[o:o + n_] = r
        self.want[self.int_entry[1]:self.int_entry[1] + nb] = _u8(ints).ravel()
        # device
        self.blob_dev = torch.full((self.live.total,), 7.0,
                                   dtype=torch.bfloat16, device=self.dev)
        self.arena = torch.full((self.size,), 0xFF, dtype=torch.uint8,
                                device=self.dev)
        self.tbl = torch.from_numpy(np.concatenate(
            [self.table.view(np.uint8),
             self.tile_start.view(np.uint8)])).to(self.dev)
        self.stream = torch.cuda.Stream(device=self.dev)
        torch.cuda.synchronize()

    def args(self, **over):
        n = len(self.table)
        a = dict(stream=self.stream.cuda_stream,
                 blob_dev=self.blob_dev.data_ptr(),
                 blob_pinned=self.blob_pin.data_ptr(),
                 blob_bytes=self.live.total * 2,
                 arena_dev=self.arena.data_ptr(), arena_bytes=self.size,
                 arena_pinned=self.rem_pin.data_ptr(),
                 pinned_bytes=self.rem_pin.numel(), spans=self.spans,
                 table=self.tbl.data_ptr(), n_entries=n,
                 tile_start=self.tbl.data_ptr() + n * 40,
                 total_tiles=int(self.tile_start[-1]))
        a.update(over)
        return tuple(a.values())

    def device_bytes(self):
        torch.cuda.synchronize()
        return _u8(self.blob_dev.cpu()), self.arena.cpu().numpy()


@pytest.mark.gpu
def test_restore_weights_on_a_hand_made_plan():
    c = _Restore()
    assert len(c.table) == len(HAND_MADE)
    c.ext.restore_weights(*c.args())
    blob, arena = c.device_bytes()
    assert np.array_equal(blob, _u8(c.cblob))
    for (key, o, nb, _d, _s), r in zip(c.entries, c.want_regions):
        assert np.array_equal(arena[o:o + nb], r), key
    io, inb = c.int_entry[1], c.int_entry[2]
    assert np.array_equal(arena[io:io + inb], c.want[io:io + inb])
    bad = np.nonzero(arena != c.want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    # the vector kernels read in place sits at its compact offset
    o, n = c.live.slots[c.vec]
    got = c.blob_dev[o:o + n].float().cpu().numpy()
    want = torch.from_numpy(c.plan.tensors[c.vec].weight).to(
        torch.bfloat16).float().numpy()
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_restore_weights_with_a_cached_blob_and_no_arena():
    c = _Restore()
    c.ext.restore_weights(*c.args(
        arena_dev=0, arena_bytes=0, arena_pinned=0, pinned_bytes=0,
        spans=[], table=0, n_entries=0, tile_start=0, total_tiles=0))
    blob, arena = c.device_bytes()
    assert np.array_equal(blob, _u8(c.cblob))
    assert (arena == 0xFF).all()


@pytest.mark.gpu
def test_restore_weights_throws_before_it_enqueues():
    c = _Restore()
    blob0, arena0 = c.device_bytes()
    past = [(c.size - 64, 256, 148)]
    for over in (dict(blob_dev=0), dict(blob_pinned=0), dict(arena_dev=0),
                 dict(arena_pinned=0), dict(table=0), dict(tile_start=0),
                 dict(spans=past), dict(spans=[(0, 1024 - 64, 148)]),
                 dict(spans=[(-256, 256, 148)]),
                 dict(spans=[(0, 256, -148)]),
                 dict(spans=[(2 ** 62, 256, 2 ** 62)]),
                 dict(n_entries=2, total_tiles=1),
                 dict(n_entries=-1, total_tiles=-1),
                 dict(blob_bytes=-1), dict(arena_bytes=-1),
                 dict(pinned_bytes=-1)):
        with pytest.raises(RuntimeError):
            c.ext.restore_weights(*c.args(**over))
    # every other argument was valid each time: a copy enqueued before
    # the check would have landed
    blob1, arena1 = c.device_bytes()
    assert np.array_equal(blob0, blob1) and np.array_equal(arena0, arena1)


# -- GPU: the pool / loader path -------------------------------------------
def _forget_plan_caches(gpu):
    with gpu._tmpl_lock:
        gpu._transform_arenas.clear()
        gpu._arena_order.clear()
        gpu._ctx_templates.clear()
        gpu._tmpl_order.clear()


def _hardlinked_repo(tmp_path, builder, kw, n):
    from tfservingcache_amd.models import write_model_repo
    repo = tmp_path / "repo"
    write_model_repo(str(repo), [("m0", 1, builder)], {"m0": kw})
    for i in range(1, n):
        dst = repo / f"m{i}" / "1"
        os.makedirs(dst.parent, exist_ok=True)
        shutil.copytree(repo / "m0" / "1", dst, copy_function=os.link)
    return repo


def _count_restores(monkeypatch, gpu):
    _t, ext = gpu._load_backend()
    calls = []
    native = ext.restore_weights

    def counted(*a):
        calls.append(a)
        return native(*a)
    monkeypatch.setattr(ext, "restore_weights", counted)
    return calls


@pytest.mark.gpu
def test_repeat_loads_go_through_restore_weights(tmp_path, monkeypatch):
    from tfservingcache_amd.cachemanager import (CacheManager, LRUCache,
                                                 ModelPool, make_gpu_loader)
    from tfservingcache_amd.cachemanager.providers import DiskModelProvider
    from tfservingcache_amd.engine import gpu
    from tfservingcache_amd.engine.model import load_model_from_dir

    repo = _hardlinked_repo(tmp_path, "resnet50",
                            dict(image_size=32, num_classes=10), 4)
    cache = LRUCache(str(tmp_path / "cache"), 10 ** 9)
    pool = ModelPool(make_gpu_loader(cache, max_batch=8, prewarm_batch=2),
                     max_concurrent_models=4)
    cm = CacheManager(DiskModelProvider(str(repo)), cache, pool)
    x = np.random.default_rng(0).standard_normal(
        (2, 32, 32, 3)).astype(np.float32) * 0.3
    _forget_plan_caches(gpu)
    monkeypatch.setenv("TFSC_GPU_LAYOUT", "on")
    calls = _count_restores(monkeypatch, gpu)

    first = cm.ensure_loaded("m0", 1)
    assert not calls and not first._gpu.restored_by_kernel
    live = emit.live_blob_layout(first._gpu.plan)
    assert first._gpu._weight_blob.numel() == live.total
    assert gpu._blob_cache_get(first._gpu.plan).numel() == live.total
    _entries, host = gpu._get_transform_arena(first._gpu.plan, "bf16")
    assert host.n_entries > 50
    out_first = first.predict({"input": x})["probs"]

    outs = []
    for n, name in enumerate(("m1", "m2"), 1):
        lm = cm.ensure_loaded(name, 1)
        assert len(calls) == n and lm._gpu.restored_by_kernel
        # blob bytes, arena bytes, layout entries of the one call
        assert calls[-1][3] == live.total * 2
        assert calls[-1][5] == host.total
        assert calls[-1][10] == host.n_entries
        assert lm._gpu.weight_bytes() == live.total * 2 + host.total
        outs.append(lm.predict({"input": x})["probs"])
    assert np.array_equal(outs[0], outs[1])
    np.testing.assert_allclose(outs[0], out_first, rtol=0.05, atol=0.02)
    cpu = load_model_from_dir(str(repo / "m0" / "1"), "cpu", 1)
    want = cpu.predict({"input": x})["probs"]
    np.testing.assert_allclose(outs[0], want, rtol=0.05, atol=0.02)
    # a dead weight is no master weight, like an index the plan lacks
    dead = next(i for i in emit.blob_layout(first._gpu.plan).slots
                if i not in live.slots)
    assert not first._gpu.has_master_weight(dead)
    with pytest.raises(KeyError):
        first._gpu.master_weight(dead)
    _forget_plan_caches(gpu)


@pytest.mark.gpu
def test_fp8_repeat_load_restores_from_pinned_spans(tmp_path, monkeypatch):
    from tfservingcache_amd.cachemanager import (CacheManager, LRUCache,
                                                 ModelPool, make_gpu_loader)
    from tfservingcache_amd.cachemanager.providers import DiskModelProvider
    """The small BERT of the CPU fixtures with one head instead of two:
    with heads=2 its head_dim is 32, and the engine's batched GEMM takes
    K in multiples of 64 only ("gemm: K must be a multiple of 64 (got
    32)" from the first load's warm-up run, before any restore). One head
    of 64 is the nearest BERT the engine serves; the weights, the fp8
    regions and the arena are of the same sizes."""
    from tfservingcache_amd.engine import gpu

    repo = _hardlinked_repo(tmp_path, "bert_base",
                            dict(seq_len=16, hidden=64, layers=1, heads=1,
                                 intermediate=200, vocab=99), 3)
    cache = LRUCache(str(tmp_path / "cache"), 10 ** 9)
    pool = ModelPool(make_gpu_loader(cache, max_batch=8, prewarm_batch=2,
                                     dtype="fp8"),
                     max_concurrent_models=3)
    cm = CacheManager(DiskModelProvider(str(repo)), cache, pool)
    ids = np.random.default_rng(0).integers(0, 99, (2, 16)).astype(np.int32)
    _forget_plan_caches(gpu)
    monkeypatch.setenv("TFSC_GPU_LAYOUT", "on")
    calls = _count_restores(monkeypatch, gpu)

    first = cm.ensure_loaded("m0", 1)
    assert not calls
    entries, host = gpu._get_transform_arena(first._gpu.plan, "fp8")
    f8 = [e for e in entries if e[0][0] in ("f8q", "f8s")]
    assert f8 and host.pinned is not None
    assert sum(s[2] for s in host.spans) >= sum(e[2] for e in f8)
    outs = []
    for n, name in enumerate(("m1", "m2"), 1):
        lm = cm.ensure_loaded(name, 1)
        assert len(calls) == n and calls[-1][8] == host.spans
        assert getattr(lm._gpu, "_arena_dev", None) is not None
        outs.append(lm.predict({"input_ids": ids}))
    assert outs[0].keys() == outs[1].keys() and outs[0]
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all()
        assert np.array_equal(outs[0][k], outs[1][k]), k
    _forget_plan_caches(gpu)

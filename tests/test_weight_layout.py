"""The weight-layout descriptor table (engine/emit.py) and its kernel
(csrc/ops/weight_layout.hip).

A repeat cold load fills its transform arena from the bf16 master blob on
the GPU. What it must reproduce, byte for byte, are the torch expressions
of GpuModel.conv_weight / conv_weight_cpad / gemm_weight; they are written
out again here (`ref_*`) and run on CPU tensors for the table tests and on
the device for the kernel test. `interpret` is a numpy reading of a table,
independent of the kernel's tiling.
"""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.planner import Plan, PlanTensor, compile_graph
from tfservingcache_amd.models import builders


# -- the reference: gpu.py's transforms, on whatever device w lives --------
def _pad_k(w):
    n, k = w.shape
    kp = emit._pad64(k)
    if kp != k:
        w = torch.nn.functional.pad(w, (0, kp - k))
    return w.to(torch.bfloat16).contiguous()


def ref_gemm(w, trans_b):
    w = w.float()
    if not trans_b:
        w = w.t().contiguous()
    return _pad_k(w)


def ref_conv(w):
    w = w.float()
    R, S, C, Kc = w.shape
    return _pad_k(w.reshape(R * S * C, Kc).t().contiguous())


def ref_cpad(w, c8):
    w = w.float()
    R, S, C, Kc = w.shape
    w = torch.nn.functional.pad(w, (0, 0, 0, c8 - C))
    return _pad_k(w.reshape(R * S * c8, Kc).t().contiguous())


def ref_region(w, key):
    if key[0] == "gw":
        return ref_gemm(w, key[2])
    if len(key) == 2:
        return ref_conv(w)
    return ref_cpad(w, key[3])


# -- a blob, an arena and its entries, as engine/gpu.py lays them out ------
def make_blob(plan):
    """bf16 master blob of a plan on the CPU (slot padding zero)."""
    layout = emit.blob_layout(plan)
    blob = torch.zeros(layout.total, dtype=torch.bfloat16)
    for idx, (off, n) in layout.slots.items():
        w = np.array(plan.tensors[idx].weight, dtype=np.float32)
        blob[off:off + n] = torch.from_numpy(w).view(-1)   # f32 -> bf16
    return layout, blob


def make_arena(plan, layout, blob, keys):
    """(entries, expected arena bytes with 0xFF wherever no entry lies):
    regions in `keys` order at _pad256b offsets, like
    publish_transform_arena."""
    entries, refs, off = [], [], 0
    for key in keys:
        o, n = layout.slots[key[1]]
        w = blob[o:o + n].view(tuple(plan.tensors[key[1]].weight.shape))
        r = ref_region(w, key)
        nb = r.numel() * 2
        entries.append((key, off, nb, torch.bfloat16, tuple(r.shape)))
        refs.append(r)
        off = emit._pad256b(off + nb)
    want = np.full(off, 0xFF, np.uint8)
    for (_k, o, nb, _d, _s), r in zip(entries, refs):
        want[o:o + nb] = r.view(torch.int16).numpy().view(np.uint8).ravel()
    return entries, want


def interpret(table, blob_u16, arena_u8):
    """Write every entry of `table` into arena_u8 from blob_u16."""
    for e in table:
        rin, cin, kp = int(e["rin"]), int(e["cin"]), int(e["kp"])
        s = int(e["src_off"])
        src = blob_u16[s:s + rin * cin].reshape(rin, cin)
        if e["transpose"]:
            k = np.arange(kp)
            q, c = k // int(e["c_dst"]), k % int(e["c_dst"])
            sr = q * int(e["c_src"]) + c
            live = (c < int(e["c_src"])) & (sr < rin)
            dst = np.zeros((cin, kp), np.uint16)
            dst[:, live] = src[sr[live], :].T
        else:
            dst = np.zeros((rin, kp), np.uint16)
            dst[:, :cin] = src
        d = int(e["dst_off"])
        arena_u8[d:d + dst.size * 2] = dst.view(np.uint8).ravel()


def _compile(builder, **kw):
    mg = builder(seed=0, **kw).meta_graphs[0]
    return compile_graph(mg.graph_def, next(iter(mg.signature_def.values())))


@functools.lru_cache(maxsize=None)
def _model_case(name):
    plan = {
        "resnet": lambda: _compile(builders.build_resnet50, image_size=32,
                                   num_classes=10),
        "bert": lambda: _compile(builders.build_bert, seq_len=16, hidden=64,
                                 layers=1, heads=2, intermediate=200,
                                 vocab=99),
    }[name]()
    keys = [k for k in emit.build_template(plan, 2, "bf16").region_keys
            if k[0] in ("gw", "cw")]
    layout, blob = make_blob(plan)
    entries, want = make_arena(plan, layout, blob, keys)
    return plan, layout, blob, keys, entries, want


@pytest.mark.parametrize("name", ["resnet", "bert"])
def test_table_reproduces_the_torch_transforms(name):
    plan, layout, blob, keys, entries, want = _model_case(name)
    assert keys
    kinds = {(k[0],) + tuple(k[2:3]) for k in keys}
    assert kinds >= ({("cw",), ("cw", "cpad")} if name == "resnet"
                     else {("gw", False)})
    table, tile_start, covered = emit.weight_layout_table(plan, entries)
    assert covered == set(keys) and len(table) == len(keys)
    got = np.full(len(want), 0xFF, np.uint8)
    interpret(table, blob.view(torch.int16).numpy().view(np.uint16), got)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["resnet", "bert"])
def test_table_tiles_the_arena(name):
    plan, layout, _blob, _keys, entries, want = _model_case(name)
    table, tile_start, _ = emit.weight_layout_table(plan, entries)
    emit.check_layout_table(table, tile_start, layout.total, len(want))
    assert table.dtype.itemsize == 40
    assert tile_start.dtype == np.int32 and tile_start[0] == 0
    spans = []
    for e, ent, t0, t1 in zip(table, entries, tile_start, tile_start[1:]):
        rows = int(e["cin"] if e["transpose"] else e["rin"])
        nb = rows * int(e["kp"]) * 2
        assert e["dst_off"] % 256 == 0 and e["kp"] % 64 == 0
        assert (int(e["dst_off"]), nb) == (ent[1], ent[2])
        assert t1 - t0 == -(-rows // 64) * (int(e["kp"]) // 64) >= 1
        spans.append((int(e["dst_off"]), int(e["dst_off"]) + nb))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] <= len(want)


def test_regions_that_are_no_relayout_stay_out_of_the_table():
    plan, layout, _blob, keys, entries, _want = _model_case("bert")
    extra = [(("int", 0), 1 << 20, 64, torch.int32, (16,)),
             (("f8q",) + keys[0][1:], 2 << 20, 128, torch.uint8, (1, 128)),
             (keys[0], 3 << 20, entries[0][2] + 2, torch.bfloat16, ())]
    table, _ts, covered = emit.weight_layout_table(plan, extra)
    assert len(table) == 0 and not covered


def test_check_layout_table_refuses_bad_tables():
    plan, layout, _blob, _keys, entries, want = _model_case("bert")
    table, tile_start, _ = emit.weight_layout_table(plan, entries)
    n = len(want)
    for field, value in (("src_off", layout.total), ("dst_off", n),
                         ("dst_off", int(table[0]["dst_off"]) + 2),
                         ("kp", int(table[0]["kp"]) + 1),
                         ("rin", int(table[0]["rin"]) + 64)):
        bad = table.copy()
        bad[0][field] = value
        with pytest.raises(ValueError):
            emit.check_layout_table(bad, tile_start, layout.total, n)
    if len(table) > 1:
        bad = table.copy()
        bad[1]["dst_off"] = bad[0]["dst_off"]
        with pytest.raises(ValueError):
            emit.check_layout_table(bad, tile_start, layout.total, n)
    with pytest.raises(ValueError):
        emit.check_layout_table(table, tile_start[:-1], layout.total, n)


# -- the kernel ------------------------------------------------------------
# (key kind, master shape, extra): the smallest shapes at which each path
# can go wrong
HAND_MADE = [
    ("cw", (7, 7, 3, 64), None),        # R*S*C = 147 -> 192, ragged both ways
    ("cpad", (7, 7, 3, 64), 8),         # the same weight, 392 -> 448
    ("cw", (1, 1, 64, 64), None),       # exactly one tile, no pad
    ("cw", (3, 3, 8, 1), None),         # one output channel
    ("cw", (1, 1, 1, 1), None),         # degenerate
    ("gw", (2048, 1000), False),        # N not a tile multiple
    ("gw", (70, 130), False),           # K -> 128, both ragged
    ("gw", (10, 100), True),            # copy path with pad
]


def _hand_made_plan():
    rng = np.random.default_rng(7)
    tensors, keys, seen = [], [], {}
    for kind, shape, extra in HAND_MADE:
        idx = seen.get(shape)
        if idx is None:
            idx = seen[shape] = len(tensors)
            tensors.append(PlanTensor(
                idx, shape, "f32", "weight", weight=rng.standard_normal(
                    shape).astype(np.float32)))
        keys.append(("gw", idx, extra) if kind == "gw" else
                    ("cw", idx) if kind == "cw" else
                    ("cw", idx, "cpad", extra))
    return Plan(tensors, [], {}, {}, {}), keys


@pytest.mark.gpu
def test_kernel_matches_torch_on_hand_made_entries():
    from tfservingcache_amd.engine.gpu import _load_backend
    _torch, ext = _load_backend()
    plan, keys = _hand_made_plan()
    layout, blob = make_blob(plan)
    dev = "cuda:0"
    blob_d = blob.to(dev)
    # the reference transform runs on the device, like a first load's
    entries, refs, off = [], [], 0
    for key in keys:
        o, n = layout.slots[key[1]]
        r = ref_region(blob_d[o:o + n].view(
            tuple(plan.tensors[key[1]].weight.shape)), key)
        entries.append((key, off, r.numel() * 2, torch.bfloat16,
                        tuple(r.shape)))
        refs.append(r)
        off = emit._pad256b(off + r.numel() * 2)
    want = torch.full((off,), 0xFF, dtype=torch.uint8, device=dev)
    for (_k, o, nb, _d, _s), r in zip(entries, refs):
        want[o:o + nb] = r.view(torch.uint8).reshape(-1)
    table, tile_start, covered = emit.weight_layout_table(plan, entries)
    assert covered == set(keys)
    emit.check_layout_table(table, tile_start, layout.total, off)
    assert len({int(b) - int(a) for a, b in
                zip(tile_start, tile_start[1:])}) > 3
    # the CPU reading of the table agrees before anything is launched
    cpu = np.full(off, 0xFF, np.uint8)
    interpret(table, blob.view(torch.int16).numpy().view(np.uint16), cpu)
    assert np.array_equal(cpu, want.cpu().numpy())

    tbl = torch.from_numpy(np.concatenate(
        [table.view(np.uint8), tile_start.view(np.uint8)])).to(dev)
    arena = torch.full((off,), 0xFF, dtype=torch.uint8, device=dev)
    ext.weight_layout(blob_d.data_ptr(), arena.data_ptr(), tbl.data_ptr(),
                      len(table), tbl.data_ptr() + len(table) * 40,
                      int(tile_start[-1]))
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    exp = want.cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"


@pytest.mark.gpu
def test_launcher_refuses_empty_or_null():
    from tfservingcache_amd.engine.gpu import _load_backend
    _torch, ext = _load_backend()
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    p = t.data_ptr()
    with pytest.raises(RuntimeError):
        ext.weight_layout(p, p, p, 0, p, 0)
    with pytest.raises(RuntimeError):
        ext.weight_layout(0, p, p, 1, p, 1)
    with pytest.raises(RuntimeError):
        ext.weight_layout(p, p, p, 2, p, 1)


@pytest.mark.gpu
def test_repeat_load_restores_through_the_kernel(tmp_path, monkeypatch):
    """Pool/loader path of the headline bench: the second load of a plan
    fills its arena with the kernel; the bytes of every region and a
    batch-2 predict equal those of a repeat load whose arena was published
    with the switch off (full pinned snapshot, second DMA)."""
    from tfservingcache_amd.cachemanager import (CacheManager, LRUCache,
                                                 ModelPool, make_gpu_loader)
    from tfservingcache_amd.cachemanager.providers import DiskModelProvider
    from tfservingcache_amd.engine import gpu
    from tfservingcache_amd.models import write_model_repo

    repo = tmp_path / "repo"
    write_model_repo(str(repo), [("m0", 1, "resnet50")],
                     {"m0": dict(image_size=32, num_classes=10)})
    for i in (1, 2, 3):
        dst = repo / f"m{i}" / "1"
        os.makedirs(dst.parent, exist_ok=True)
        shutil.copytree(repo / "m0" / "1", dst, copy_function=os.link)
    cache = LRUCache(str(tmp_path / "cache"), 10 ** 9)
    pool = ModelPool(make_gpu_loader(cache, max_batch=8, prewarm_batch=2),
                     max_concurrent_models=4)
    cm = CacheManager(DiskModelProvider(str(repo)), cache, pool)
    x = np.random.default_rng(0).standard_normal(
        (2, 32, 32, 3)).astype(np.float32) * 0.3

    def forget_plan_caches():
        # a fresh process for this plan, as far as engine/gpu.py goes
        with gpu._tmpl_lock:
            gpu._transform_arenas.clear()
            gpu._arena_order.clear()
            gpu._ctx_templates.clear()
            gpu._tmpl_order.clear()

    def regions(gm):
        torch.cuda.synchronize()
        a = gm._arena_dev.cpu().numpy()
        return {k: a[e[1]:e[1] + e[2]].copy()
                for k, e in gm._arena_entries.items()}

    forget_plan_caches()
    monkeypatch.setenv("TFSC_GPU_LAYOUT", "on")
    first = cm.ensure_loaded("m0", 1)
    assert not first._gpu.restored_by_kernel
    entries, host = gpu._get_transform_arena(first._gpu.plan, "bf16")
    # no transform bytes in pinned memory: only the int weights (the
    # reduction axes of the global mean) are still a host copy
    n_int = sum(emit._pad256b(e[2]) for e in entries if e[0][0] == "int")
    assert host.n_entries == sum(e[0][0] in ("gw", "cw") for e in entries)
    assert host.n_entries > 50
    assert (0 if host.pinned is None else host.pinned.numel()) == n_int
    assert sum(s[2] for s in host.spans) == n_int < 4096
    on = cm.ensure_loaded("m1", 1)
    assert on._gpu.restored_by_kernel
    out_first = first.predict({"input": x})["probs"]
    out_on = on.predict({"input": x})["probs"]

    forget_plan_caches()
    monkeypatch.setenv("TFSC_GPU_LAYOUT", "off")
    cm.ensure_loaded("m2", 1)
    host = gpu._get_transform_arena(first._gpu.plan, "bf16")[1]
    assert host.n_entries == 0 and host.pinned.numel() == host.total
    off = cm.ensure_loaded("m3", 1)
    assert getattr(off._gpu, "_arena_dev", None) is not None
    assert not off._gpu.restored_by_kernel
    out_off = off.predict({"input": x})["probs"]

    r_on, r_off = regions(on._gpu), regions(off._gpu)
    assert r_on.keys() == r_off.keys() and len(r_on) > 50
    assert on._gpu.weight_bytes() == off._gpu.weight_bytes()
    for k in r_on:
        assert np.array_equal(r_on[k], r_off[k]), k
    assert np.array_equal(out_on, out_off)
    # the first load's torch-made transforms hold the same bytes; its
    # eager-then-captured run is not required to match bit for bit
    np.testing.assert_allclose(out_on, out_first, rtol=0.05, atol=0.02)
    forget_plan_caches()

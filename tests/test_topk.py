"""TopKV2 on the CPU side: planner lowering, the CPU executor's
definition, and the call the emitter makes (ARGMAX_LAST's 4-pointer /
4-int form). The kernel itself is pinned in test_gpu_topk.py."""
import numpy as np
import pytest

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.executor_cpu import CpuExecutor
from tfservingcache_amd.engine.planner import PlanError, compile_graph
from tfservingcache_amd.engine.savedmodel import GraphBuilder


def _plan(op="TopKV2", k=3, shape=(-1, 4, 9), dtype=np.float32,
          const_k=True, argmax=False, **attrs):
    gb = GraphBuilder()
    f32, i32, i64 = gb.a_type(1), gb.a_type(3), gb.a_type(9)
    x = gb.placeholder("x", dtype, list(shape), signature_name="x")
    if op == "TopK":
        top = gb.node("TopK", "top", [x], T=f32, k=gb.a_int(k), **attrs)
    else:
        kk = gb.const("k", np.int32(k)) if const_k else \
            gb.placeholder("kin", np.int32, [], signature_name="kin")
        top = gb.node("TopKV2", "top", [x, kk], T=f32,
                      index_type=i64, **attrs)
    gb.mark_output("values", f"{top}:0")
    gb.mark_output("indices", f"{top}:1")
    if argmax:
        gb.mark_output("best", gb.node(
            "ArgMax", "am", [x, gb.const("ax", np.int32(-1))], T=f32,
            output_type=i32))
    mg = gb.build().meta_graphs[0]
    return compile_graph(mg.graph_def,
                         next(iter(mg.signature_def.values())))


@pytest.mark.parametrize("op,attrs", [
    ("TopKV2", {}), ("TopK", {}),
    ("TopKV2", {"sorted": GraphBuilder.a_bool(False)})])
def test_planner_lowers_to_one_topk_last(op, attrs):
    plan = _plan(op=op, **attrs)
    assert [o.kind for o in plan.ops] == ["topk_last"]
    o = plan.ops[0]
    assert o.params == {"k": 3} and len(o.inputs) == 1
    vals, idx = (plan.tensors[i] for i in o.outputs)
    assert (vals.name, vals.dtype, vals.shape) == ("top:0", "f32", (-1, 4, 3))
    assert (idx.name, idx.dtype, idx.shape) == ("top:1", "i32", (-1, 4, 3))
    assert plan.sig_outputs == {"values": vals.idx, "indices": idx.idx}


@pytest.mark.parametrize("kwargs", [
    dict(k=0), dict(k=10), dict(k=1025, shape=(-1, 2000)),
    dict(const_k=False), dict(shape=(3, -1)), dict(dtype=np.int32),
    dict(op="TopK", k=0)],
    ids=["k<1", "k>cols", "k>1024", "dynamic-k", "symbolic-cols",
         "int-input", "TopK-attr-k<1"])
def test_planner_refuses(kwargs):
    with pytest.raises(PlanError):
        _plan(**kwargs)


def test_cpu_executor_is_the_stable_descending_order():
    # ties, a tie that straddles the cut at k, +0.0 before -0.0 and after
    x = np.array([[1.0, 5.0, -0.0, 5.0, 0.0, 1.0, -np.inf, 1.0],
                  [0.0, -0.0, -1.0, -0.0, 0.0, -2.0, -1.0, -3.0]],
                 np.float32).reshape(2, 1, 8)
    plan = _plan(k=5, shape=(-1, 1, 8))
    out = CpuExecutor(plan).run({plan.sig_inputs["x"]: x}, 2,
                                list(plan.sig_outputs.values()))
    idx = out[plan.sig_outputs["indices"]]
    vals = out[plan.sig_outputs["values"]]
    assert idx.dtype == np.int32 and vals.dtype == np.float32
    np.testing.assert_array_equal(
        idx.reshape(2, 5), [[1, 3, 0, 5, 7], [0, 1, 3, 4, 2]])
    # the element's own bits: -0.0 comes back as -0.0
    np.testing.assert_array_equal(
        vals.view(np.uint32), np.take_along_axis(x, idx, -1).view(np.uint32))


def test_emitter_extends_argmax_last():
    # no new call kind: the 24 the golden templates reach
    assert len(emit.KINDS) == 24 and not any("TOP" in k for k in emit.KINDS)
    plan = _plan(argmax=True)
    tmpl = emit.build_template(plan, 2, "bf16")
    (topk, argmax) = tmpl.calls
    o = plan.ops[0]
    ws = lambda i: (emit.WS, tmpl.bufs[tmpl.root[i]].offset)    # noqa: E731
    assert topk[1] == [ws(o.inputs[0]), ws(o.outputs[1]), ws(o.outputs[0]),
                       None]
    assert topk[2] == [8, 9, 3, 1] and topk[3] == []
    # values are bf16, indices i32, in the workspace
    assert tmpl.bufs[o.outputs[0]].nbytes == 8 * 3 * 2
    assert tmpl.bufs[o.outputs[1]].nbytes == 8 * 3 * 4
    assert tmpl.bufs[o.outputs[1]].is_int
    # a plain ArgMax is still today's call
    assert len(argmax[1]) == 2 and argmax[2] == [8, 9]


def test_emitter_sizes_the_scratch_of_a_split_row():
    rows, cols, k = 1, 1_000_000, 10
    P = emit.topk_segments(rows, cols, k)
    assert P > 1 and (P - 1) * -(-cols // P) < cols    # no empty segment
    assert emit.topk_segments(64, 1000, k) == 1
    plan = _plan(k=k, shape=(-1, cols))
    tmpl = emit.build_template(plan, rows, "bf16")
    (call,) = tmpl.calls
    assert call[2] == [rows, cols, k, P]
    off = tmpl.scratch_off[0]
    assert call[1][3] == (emit.WS, off) and off % 8 == 0
    assert off + rows * P * k * 8 <= tmpl.total_bytes
    assert all(off >= b.offset + b.nbytes or
               off + rows * P * k * 8 <= b.offset for b in tmpl.bufs.values())

"""BlockLSTM / BlockLSTMV2 on the CPU side: the planner's lowering to one
`lstm` op, the CPU executor against a plain fp64 LSTM, and the calls the
emitter makes (GEMM, then LSTM). The kernels are pinned in
test_gpu_lstm.py."""
import numpy as np
import pytest

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.executor_cpu import CpuExecutor
from tfservingcache_amd.engine.planner import (PlanError, compile_graph,
                                               lstm_cols, lstm_unpack)
from tfservingcache_amd.engine.savedmodel import GraphBuilder

T, I, H = 5, 6, 20
GATES = {"BlockLSTM": "icfo", "BlockLSTMV2": "ifco"}     # c = ci


def reference(x, w, b, gates, forget_bias=0.0, clip=0.0, peep=None,
              h0=None, c0=None, rnd=lambda v: v):
    """Plain fp64 LSTM on TF's [I+H, 4H] weight. x is [T,B,I]; `gates` is
    the op's column order; `rnd` rounds pre and each h (the two roundings
    the GPU design makes; identity on the CPU). Returns (h, cs) [T,B,H]."""
    x, w, b = (np.asarray(v, np.float64) for v in (x, w, b))
    n_t, n_b, n_i = x.shape
    n_h = w.shape[1] // 4
    sl = {g: slice(k * n_h, (k + 1) * n_h) for k, g in enumerate(gates)}
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))             # noqa: E731
    wci, wcf, wco = peep if peep is not None else (np.zeros(n_h),) * 3
    h = np.zeros((n_b, n_h)) if h0 is None else np.asarray(h0, np.float64)
    c = np.zeros((n_b, n_h)) if c0 is None else np.asarray(c0, np.float64)
    bias = b.copy()
    bias[sl["f"]] += forget_bias
    pre = rnd(x @ w[:n_i] + bias)
    hs, cs = np.empty((n_t, n_b, n_h)), np.empty((n_t, n_b, n_h))
    for t in range(n_t):
        z = pre[t] + h @ w[n_i:]
        i, f = sig(z[:, sl["i"]] + c * wci), sig(z[:, sl["f"]] + c * wcf)
        c = np.tanh(z[:, sl["c"]]) * i + c * f
        if clip > 0:
            c = np.clip(c, -clip, clip)
        h = rnd(sig(z[:, sl["o"]] + c * wco) * np.tanh(c))
        hs[t], cs[t] = h, c
    return hs, cs


def _weights(seed=0):
    rng = np.random.default_rng(seed)
    return {"w": rng.standard_normal((I + H, 4 * H)).astype(np.float32) * .3,
            "b": rng.standard_normal(4 * H).astype(np.float32) * 0.3,
            "peep": [rng.standard_normal(H).astype(np.float32) * 0.5
                     for _ in range(3)]}


def _plan(op="BlockLSTM", peephole=False, clip=0.0, forget_bias=1.0,
          batch_major=False, fill=True, seq_len=T, out=6, w_shape=None,
          b_shape=None, w_const=True, want_cs=False):
    """x -> [Transpose] -> op -> [Transpose] as signature output `y`."""
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    ws = _weights()

    def c(name, v, dtype=np.float32):
        return gb.const(name, np.asarray(v, dtype=dtype))

    swap = c("swap", [1, 0, 2], np.int32)
    x = gb.placeholder("x", np.float32, [-1, T, I] if batch_major
                       else [T, -1, I], signature_name="x")
    if batch_major:
        x = gb.node("Transpose", "tm", [x, swap], T=f32, Tperm=i32)
    if fill:
        h0 = c0 = gb.node("Fill", "zeros", [c("dims", [-1, H], np.int32),
                                            c("zero", 0.0)], T=f32)
    else:
        h0 = gb.placeholder("h0", np.float32, [-1, H], signature_name="h0")
        c0 = gb.placeholder("c0", np.float32, [-1, H], signature_name="c0")
    slm = c("slm", seq_len, np.int64) if seq_len is not None else \
        gb.placeholder("slm", np.int32, [], signature_name="slm")
    w = c("w", ws["w"] if w_shape is None else np.zeros(w_shape)) \
        if w_const else gb.placeholder("w", np.float32, [I + H, 4 * H],
                                       signature_name="w")
    attrs = {"cell_clip": gb.a_float(clip),
             "use_peephole": gb.a_bool(peephole)}
    if op == "BlockLSTM":
        attrs["forget_bias"] = gb.a_float(forget_bias)
    node = gb.node(op, "lstm", [
        slm, x, c0, h0, w, *(c(n, v) for n, v in zip(("wci", "wcf", "wco"),
                                                      ws["peep"])),
        c("b", ws["b"] if b_shape is None else np.zeros(b_shape))],
        T=f32, **attrs)
    y = f"{node}:{out}"
    if batch_major:
        y = gb.node("Transpose", "bm", [y, swap], T=f32, Tperm=i32)
    gb.mark_output("y", y)
    if want_cs:
        gb.mark_output("cs", f"{node}:1")
    mg = gb.build().meta_graphs[0]
    return compile_graph(mg.graph_def,
                         next(iter(mg.signature_def.values()))), ws


@pytest.mark.parametrize("op", list(GATES))
def test_lowering_normalises_gates_and_bias(op):
    plan, ws = _plan(op=op, forget_bias=0.75)
    assert [o.kind for o in plan.ops] == ["lstm"]      # the Fill is consumed
    o = plan.ops[0]
    assert o.params == {"T": T, "I": I, "H": H, "cell_clip": 0.0,
                        "peephole": False, "h0": False, "c0": False,
                        "cs": False, "x_batch_major": False,
                        "h_batch_major": False}
    wx, wh, b = (plan.tensors[i].weight for i in o.inputs[1:])
    assert wx.shape == (I, lstm_cols(H)) and wh.shape == (H, lstm_cols(H))
    k = GATES[op].index
    order = [k("i"), k("c"), k("f"), k("o")]
    w4 = ws["w"].reshape(I + H, 4, H)[:, order]
    np.testing.assert_array_equal(lstm_unpack(wx, H), w4[:I])
    np.testing.assert_array_equal(lstm_unpack(wh, H), w4[I:])
    b4 = ws["b"].reshape(4, H)[order].copy()
    if op == "BlockLSTM":                               # V2 has no attribute
        b4[2] += np.float32(0.75)
    np.testing.assert_array_equal(lstm_unpack(b, H), b4)
    assert plan.tensors[o.outputs[0]].shape == (T, -1, H)


def test_transposes_fold_into_strides():
    plan, _ = _plan(batch_major=True)
    assert [o.kind for o in plan.ops] == ["lstm"]
    o = plan.ops[0]
    assert o.params["x_batch_major"] and o.params["h_batch_major"]
    assert plan.tensors[o.inputs[0]].name == "x:0"
    assert plan.tensors[o.outputs[0]].shape == (-1, T, H)
    assert plan.sig_outputs["y"] == o.outputs[0]
    # cs wanted: it would share h's strides, so the output stays time-major
    plan, _ = _plan(batch_major=True, want_cs=True)
    assert [o.kind for o in plan.ops] == ["lstm", "transpose"]
    assert not plan.ops[0].params["h_batch_major"]


def test_transpose_between_two_layers_folds_once():
    """A Transpose that is layer 1's sole h consumer and layer 2's x folds
    into layer 1 only; layer 2 then sees [B,T,H] as time-major, which the
    symbolic batch makes a PlanError naming it."""
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    c = lambda n, v, dt=np.float32: gb.const(n, np.asarray(v, dt))  # noqa: E731
    zeros = gb.node("Fill", "z", [c("d", [-1, H], np.int32), c("0", 0.0)])
    x = gb.placeholder("x", np.float32, [T, -1, H], signature_name="x")
    for name in ("l1", "l2"):
        node = gb.node("BlockLSTMV2", name, [
            c(f"{name}/n", T, np.int64), x, zeros, zeros,
            c(f"{name}/w", np.zeros((2 * H, 4 * H))), *(c(f"{name}/p{k}",
                                                          np.zeros(H))
                                                        for k in range(3)),
            c(f"{name}/b", np.zeros(4 * H))], T=f32)
        x = gb.node("Transpose", f"{name}/t", [f"{node}:6", c(
            f"{name}/perm", [1, 0, 2], np.int32)], T=f32, Tperm=i32)
    gb.mark_output("y", x)
    mg = gb.build().meta_graphs[0]
    with pytest.raises(PlanError, match="BlockLSTMV2 l2: T and I"):
        compile_graph(mg.graph_def, next(iter(mg.signature_def.values())))


@pytest.mark.parametrize("kwargs", [
    dict(seq_len=T - 1), dict(seq_len=None), dict(out=0),
    dict(w_const=False), dict(w_shape=(I + H + 1, 4 * H)),
    dict(b_shape=(4 * H + 4,))],
    ids=["seq_len_max<T", "dynamic-seq_len_max", "consumer-of-:0",
         "non-constant-w", "w-shape", "b-shape"])
def test_planner_refuses(kwargs):
    with pytest.raises(PlanError, match="lstm"):        # names the node
        _plan(**kwargs)


@pytest.mark.parametrize("batch_major", [False, True])
@pytest.mark.parametrize("peephole,clip", [(False, 0.0), (True, 0.2)])
@pytest.mark.parametrize("op", list(GATES))
def test_cpu_executor_vs_fp64(op, peephole, clip, batch_major):
    plan, ws = _plan(op=op, peephole=peephole, clip=clip, fill=False,
                     batch_major=batch_major, want_cs=not batch_major)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((T, 3, I)).astype(np.float32)
    h0, c0 = (rng.standard_normal((3, H)).astype(np.float32) * 0.5
              for _ in range(2))
    want_h, want_cs = reference(
        x, ws["w"], ws["b"], GATES[op], clip=clip, h0=h0, c0=c0,
        forget_bias=1.0 if op == "BlockLSTM" else 0.0,
        peep=ws["peep"] if peephole else None)
    assert not clip or (np.abs(want_cs) == clip).any()  # the clip binds
    feeds = {plan.sig_inputs["x"]: x.transpose(1, 0, 2) if batch_major else x,
             plan.sig_inputs["h0"]: h0, plan.sig_inputs["c0"]: c0}
    got = CpuExecutor(plan).run(feeds, batch=3)
    y = got[plan.sig_outputs["y"]]
    np.testing.assert_allclose(y.transpose(1, 0, 2) if batch_major else y,
                               want_h, atol=2e-6, rtol=0)
    if not batch_major:
        np.testing.assert_allclose(got[plan.sig_outputs["cs"]], want_cs,
                                   atol=4e-6, rtol=0)


def test_emitter_calls_gemm_then_lstm():
    plan, _ = _plan(peephole=True, clip=0.5, batch_major=True)
    calls = emit.build_template(plan, 4, "bf16").calls
    assert [c[0] for c in calls] == ["PAD_LAST", "GEMM", "LSTM"]
    N = lstm_cols(H)
    assert calls[1][2] == [4 * T, N, 64, 0]
    kind, ptrs, ints, floats = calls[2]
    assert ints == [T, 4, H, H, T * H, 1, T] and floats == [0.5]
    assert len(ptrs) == 10 and ptrs[0] == calls[1][1][-1]      # pre
    assert ptrs[5] is None and ptrs[6] is None and ptrs[9] is None
    assert all(p is not None for p in ptrs[:5] + ptrs[7:9])
    # time-major, no peephole
    plan, _ = _plan()
    ints = emit.build_template(plan, 3, "bf16").calls[-1][2]
    assert ints == [T, 3, H, 3 * H, H, 3, 1]

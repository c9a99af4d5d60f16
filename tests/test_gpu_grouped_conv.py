"""Grouped conv on the GPU: the grouped implicit-GEMM kernel, its
launcher's argument checks, the 15-int (dense) CONV form and
build_resnext.

Kernel level goes through ExecPlan([(K_CONV, ptrs, ints + [groups])]) on
torch bf16 tensors; the weights are laid out here as
[K][pad64(R*S*Cg)] (row g*Ng + n is group g's filter n, k = (r*S+s)*Cg+c).
The reference is torch CPU f32 conv2d(groups=) on the same bf16-rounded
values. Tolerance, derived: accumulation is f32 and the result is
rounded to bf16 once (2^-9 relative). Asserted:
|got - want| <= 2^-8 * max|want| — twice the rounding bound, the slack is
for accumulation order.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine import planner  # noqa: E402
from tfservingcache_amd.engine.model import (LoadedModel,  # noqa: E402
                                             load_model_from_dir)
from tfservingcache_amd.engine.planner import compile_graph  # noqa: E402
from tfservingcache_amd.engine.savedmodel import (  # noqa: E402
    read_saved_model, write_saved_model)
from tfservingcache_amd.models import build_resnext  # noqa: E402

SENTINEL = 1.0e30
TAIL = 64
ACT = {"none": 0, "relu": 1, "relu6": 5}


def _torch_ext():
    import torch
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return torch, ext


def _pad64(k):
    return (k + 63) // 64 * 64


def _same_pads(H, R, stride):
    Ho = -(-H // stride)
    tot = max((Ho - 1) * stride + R - H, 0)
    return Ho, tot // 2, tot - tot // 2


def _case(N, H, Cg, Ng, G, R, stride, padding, seed):
    """bf16-rounded x [N,H,H,C], w [K,Cg,R,R] (torch layout), bias [K]
    and the conv geometry."""
    torch, _ = _torch_ext()
    g = torch.Generator().manual_seed(seed)
    C, K = Cg * G, Ng * G
    x = torch.randn(N, H, H, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, Cg, R, R, generator=g) * 0.2).to(torch.bfloat16)
    b = (torch.randn(K, generator=g) * 0.5).to(torch.bfloat16)
    if padding == "SAME":
        Ho, lo, hi = _same_pads(H, R, stride)
    else:
        Ho, lo, hi = (H - R) // stride + 1, 0, 0
    return dict(N=N, H=H, C=C, K=K, Cg=Cg, G=G, R=R, stride=stride,
                Ho=Ho, lo=lo, hi=hi, x=x, w=w, b=b)


def _reference(c, act="none", res=None):
    torch, _ = _torch_ext()
    xt = torch.nn.functional.pad(c["x"].float().permute(0, 3, 1, 2),
                                 (c["lo"], c["hi"], c["lo"], c["hi"]))
    y = torch.nn.functional.conv2d(xt, c["w"].float(), c["b"].float(),
                                   stride=c["stride"], groups=c["G"])
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.float()
    if act == "relu":
        y = torch.relu(y)
    elif act == "relu6":
        y = torch.clamp(y, 0.0, 6.0)
    return y.contiguous()


def _ints(c, groups, k_pad=None, act="none"):
    R = c["R"]
    if k_pad is None:
        k_pad = _pad64(R * R * (c["C"] // groups))
    return [c["N"], c["H"], c["H"], c["C"], c["K"], R, R, c["stride"],
            c["stride"], c["lo"], c["lo"], c["Ho"], c["Ho"], k_pad,
            ACT[act]]


def _device_weight(c):
    """[K][pad64(R*R*Cg)] bf16 from the torch-layout [K,Cg,R,R]."""
    torch, _ = _torch_ext()
    K, R, cin = c["K"], c["R"], c["Cg"]
    flat = c["w"].permute(0, 2, 3, 1).reshape(K, R * R * cin)   # (r,s,c)
    out = torch.zeros(K, _pad64(R * R * cin), dtype=torch.bfloat16)
    out[:, :R * R * cin] = flat
    return out.cuda().contiguous()


def _run(c, ints, wdev, res=None):
    torch, ext = _torch_ext()
    n_out = c["N"] * c["Ho"] * c["Ho"] * c["K"]
    buf = torch.full((n_out + TAIL,), SENTINEL, dtype=torch.bfloat16,
                     device="cuda")
    x = c["x"].cuda().contiguous()
    b = c["b"].cuda().contiguous()
    zeros = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    r = res.cuda().contiguous() if res is not None else None
    ptrs = [x.data_ptr(), wdev.data_ptr(), b.data_ptr(),
            r.data_ptr() if r is not None else 0, zeros.data_ptr(),
            buf.data_ptr()]
    ext.ExecPlan([(ext.K_CONV, ptrs, ints, [])]).run()
    torch.cuda.synchronize()
    out = buf[:n_out].view(c["N"], c["Ho"], c["Ho"], c["K"]).cpu()
    return out, buf[n_out:].cpu()


def _check(c, what, act="none", with_res=False):
    torch, _ = _torch_ext()
    res = None
    if with_res:
        g = torch.Generator().manual_seed(99)
        res = torch.randn(c["N"], c["Ho"], c["Ho"], c["K"],
                          generator=g).to(torch.bfloat16)
    got, tail = _run(c, _ints(c, c["G"], act=act) + [c["G"]],
                     _device_weight(c), res)
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    assert not (got == sent).any(), f"unwritten output, {what}"
    assert (tail == sent).all(), f"wrote past the end, {what}"
    want = _reference(c, act, res)
    bound = 2.0 ** -8 * float(want.abs().max())
    err = float((got.float() - want).abs().max())
    print(f"{what}: max|err|={err:.4g} bound={bound:.4g}")
    assert err <= bound, (what, err, bound)


# (N, H, Cg, Ng, G, R, stride, padding): the smallest shapes at which each
# mechanism can go wrong
_KERNEL_CASES = {
    # half-empty MFMA column tile, K tail 72 -> 128, partial M tile (M=50)
    "ng8_ktail": (2, 5, 8, 8, 4, 3, 1, "SAME"),
    # asymmetric pad
    "s2_same": (2, 6, 16, 16, 2, 3, 2, "SAME"),
    # Ng not a multiple of 16, odd group count
    "ng24_g3_valid": (2, 7, 8, 24, 3, 3, 1, "VALID"),
    # grouped 1x1, K = 32 -> 64
    "1x1": (2, 4, 32, 32, 2, 1, 1, "VALID"),
    # several N tiles per group, the last partial
    "ng80": (2, 5, 16, 80, 2, 3, 1, "SAME"),
}


@pytest.mark.parametrize("name", list(_KERNEL_CASES))
def test_grouped_conv_kernel(name):
    c = _case(*_KERNEL_CASES[name], seed=len(name))
    _check(c, name)


@pytest.mark.parametrize("act,with_res", [("relu", True), ("relu6", False)])
def test_grouped_conv_kernel_m_tiles_epilogue(act, with_res):
    # M = 300: several M tiles, the last partial
    c = _case(3, 10, 16, 16, 4, 3, 1, "SAME", seed=5)
    _check(c, f"m300_{act}_res{int(with_res)}", act=act, with_res=with_res)


def test_grouped_conv_launcher_rejects_bad_arguments():
    torch, ext = _torch_ext()
    c = _case(2, 5, 8, 8, 4, 3, 1, "SAME", seed=1)      # C = K = 32
    x = torch.zeros(2 * 5 * 5 * 32, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(64 * 512, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(2 * 5 * 5 * 64, dtype=torch.bfloat16, device="cuda")
    ptrs = [x.data_ptr(), w.data_ptr(), w.data_ptr(), 0, w.data_ptr(),
            y.data_ptr()]
    good = _ints(c, 4)
    ext.ExecPlan([(ext.K_CONV, ptrs, good + [4], [])]).run()   # sanity
    torch.cuda.synchronize()

    def with_(groups, **kw):
        ints = list(good)
        for k, v in kw.items():
            ints[{"C": 3, "K": 4, "k_pad": 13}[k]] = v
        return ints + [groups]

    bad = [
        with_(0),                               # groups = 0
        with_(3, k_pad=_pad64(9 * 10)),         # C % groups != 0
        with_(8, k_pad=_pad64(9 * 4)),          # (C/groups) % 8 != 0
        with_(4, K=48, k_pad=_pad64(9 * 8)),    # (Kc/groups) % 8 != 0
        with_(4, k_pad=_pad64(9 * 32)),         # k_pad from the full C
    ]
    for ints in bad:
        with pytest.raises(RuntimeError):
            ext.ExecPlan([(ext.K_CONV, ptrs, ints, [])]).run()
    torch.cuda.synchronize()


def test_dense_conv_15_ints_equals_groups_1():
    """The 15-int form and a 16th int of 1 take the same (dense) path."""
    torch, _ = _torch_ext()
    c = _case(2, 7, 16, 24, 1, 3, 2, "SAME", seed=8)    # dense 16 -> 24
    wdev = _device_weight(c)
    ints = _ints(c, 1, act="relu")
    a, tail_a = _run(c, ints, wdev)
    b, tail_b = _run(c, ints + [1], wdev)
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    assert (tail_a == sent).all() and (tail_b == sent).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    want = _reference(c, "relu")
    assert float((a.float() - want).abs().max()) <= \
        2.0 ** -8 * float(want.abs().max())


# -- build_resnext: GPU vs CPU -----------------------------------------------

def _models(tmp_path):
    """(grouped on GPU, forced-dense on GPU, CPU) of one SavedModel."""
    from tfservingcache_amd.engine.gpu import GpuModel
    sm = build_resnext(image_size=32, num_classes=16,
                       stage_blocks=(1, 1, 1, 1))
    d = str(tmp_path / "rx" / "1")
    write_saved_model(sm, d)
    gm = load_model_from_dir(d, "rx", 1)
    cm = LoadedModel("rx_cpu", 1, gm.plan)
    # compiled directly: the plan cache is keyed by the SavedModel's bytes
    graph_def, sigs = read_saved_model(d)
    planner._Lowerer.GROUPED_CONV_DENSE = True
    try:
        dplan = compile_graph(graph_def, next(iter(sigs.values())))
    finally:
        planner._Lowerer.GROUPED_CONV_DENSE = False
    dm = LoadedModel("rx_dense", 1, dplan)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="rx", model_version=1)
    dm._gpu = GpuModel(dm.plan, device="cuda:0", max_batch=8,
                       model_name="rx_dense", model_version=1)
    return gm, dm, cm


def test_resnext_gpu_vs_cpu(tmp_path):
    gm, dm, cm = _models(tmp_path)
    try:
        n_grouped = [op.params.get("groups", 1) for op in gm.plan.ops
                     if op.kind == "conv2d" and "groups" in op.params]
        assert n_grouped == [8, 16, 32, 32]
        assert not any("groups" in op.params for op in dm.plan.ops)
        for batch in (2, 3):                    # 3 -> bucket 4
            x = (np.random.default_rng(batch).standard_normal(
                (batch, 32, 32, 3)) * 0.3).astype(np.float32)
            want = cm.predict({"input": x})
            got = gm.predict({"input": x})
            again = gm.predict({"input": x})    # graph replay
            dense = dm.predict({"input": x})
            assert got["probs"].shape == (batch, 16)
            assert np.all(np.isfinite(got["logits"]))
            print(f"b{batch}: max|gpu-cpu| probs="
                  f"{float(np.abs(got['probs'] - want['probs']).max()):.4g}"
                  f" max|grouped-dense| probs="
                  f"{float(np.abs(got['probs'] - dense['probs']).max()):.4g}")
            np.testing.assert_allclose(got["probs"], want["probs"],
                                       rtol=0.25, atol=0.05)
            np.testing.assert_allclose(again["probs"], got["probs"],
                                       rtol=1e-6)
            np.testing.assert_allclose(dense["probs"], got["probs"],
                                       rtol=0.25, atol=0.05)
    finally:
        gm._gpu.release()
        dm._gpu.release()

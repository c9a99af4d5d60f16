"""Timing probe for the LSTM kernels (profiles/lstm.md).

Three ways to run the recurrence of one layer over T = 64 steps, from the
same `pre` (x W_x + b, computed outside the timed region in all three):

  resident  one K_LSTM call, lstm_resident_kernel (H <= the LDS limit)
  stepped   one K_LSTM call, T launches of lstm_step_kernel
  unfused   what the engine's existing calls would need per step: one GEMM
            (h_{t-1} W_h with pre_t as the residual) and seven eltwise
            launches: sigmoid and tanh over all of z, g*i, c*f, their sum,
            tanh(c'), o*tanh(c'). The gate slices are read in place through
            ELT_BINARY's strides, so no slice copy is charged; eight
            launches a step is the least this route can do.

Every variant is one ExecPlan captured into a hipGraph. A figure is the
wall time of n back-to-back replays ending in one device synchronise,
divided by n and by T, with n sized so a sample lasts about 0.2 s; the
variants alternate, five samples each, reported as median (min - max) in
microseconds per step. capture_ms is the host time of ExecPlan.capture()
(stream capture plus instantiation) of that variant's graph.

    python scripts/lstm_probe.py [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

from conv3d_probe import BF, DEV, _alternate, _pad64, ext  # noqa: E402
from tfservingcache_amd.engine.planner import lstm_pack  # noqa: E402

T = 64


def _capture(calls, stream):
    plan = ext.ExecPlan(calls)
    with torch.cuda.stream(stream):
        plan.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.capture()
        ms = (time.perf_counter() - t0) * 1e3
        for _ in range(5):
            plan.run_graph()
        torch.cuda.synchronize()
    return plan, ms


def case(B, H, stream, rounds):
    g = torch.Generator().manual_seed(0)
    Kp = _pad64(H)
    w = (0.5 * torch.randn(H, 4, H, generator=g) / H ** 0.5)
    pre = torch.randn(T, B, 4, H, generator=g)
    # fused: packed columns; unfused: gate-major [i | ci | f | o]
    wh_p = torch.as_tensor(lstm_pack(w.numpy(), H)).t().contiguous()
    dev = {"wh_p": wh_p, "pre_p": torch.as_tensor(lstm_pack(pre.numpy(), H)),
           "wh_g": w.reshape(H, 4 * H).t().contiguous(),
           "pre_g": pre.reshape(T, B, 4 * H)}
    dev = {k: v.to(BF).to(DEV) for k, v in dev.items()}
    cstate = torch.zeros(B, H, device=DEV)
    hs = {n: torch.zeros(T, B, H, dtype=BF, device=DEV)
          for n in ("resident", "stepped", "unfused")}

    def fused(h):
        return [(ext.K_LSTM,
                 [dev["pre_p"].data_ptr(), dev["wh_p"].data_ptr(), 0, 0, 0, 0,
                  0, cstate.data_ptr(), h.data_ptr(), 0],
                 [T, B, H, B * H, H, B, 1], [0.0])]

    # unfused: z, s = sigmoid(z), tz = tanh(z) are [B,4H]; gi, cf, c, tc [B,H]
    z, s, tz = (torch.zeros(B, 4 * H, dtype=BF, device=DEV) for _ in range(3))
    gi, cf, c, tc, hzero = (torch.zeros(B, H, dtype=BF, device=DEV)
                            for _ in range(5))
    gate = lambda t, k: t.data_ptr() + k * H * 2             # noqa: E731

    def binary(fn, a, sa, b_, sb, y):
        return (ext.K_ELT_BINARY, [a, b_, y],
                [B * H, fn, 2, B, H, sa, 1, sb, 1], [])

    calls = [(ext.K_ELT_UNARY, [hzero.data_ptr(), c.data_ptr()],
              [B * H, ext.ELT_RELU], [])]                    # c = 0 per replay
    h_un = hs["unfused"]
    for t in range(T):
        hp = hzero if t == 0 else h_un[t - 1]
        calls += [
            (ext.K_GEMM, [hp.data_ptr(), dev["wh_g"].data_ptr(), 0,
                          dev["pre_g"][t].data_ptr(), z.data_ptr()],
             [B, 4 * H, Kp, 0], [1.0]),
            (ext.K_ELT_UNARY, [z.data_ptr(), s.data_ptr()],
             [B * 4 * H, ext.ELT_SIGMOID], []),
            (ext.K_ELT_UNARY, [z.data_ptr(), tz.data_ptr()],
             [B * 4 * H, ext.ELT_TANH], []),
            binary(ext.ELT_MUL, gate(tz, 1), 4 * H, gate(s, 0), 4 * H,
                   gi.data_ptr()),
            binary(ext.ELT_MUL, c.data_ptr(), H, gate(s, 2), 4 * H,
                   cf.data_ptr()),
            binary(ext.ELT_ADD, gi.data_ptr(), H, cf.data_ptr(), H,
                   c.data_ptr()),
            (ext.K_ELT_UNARY, [c.data_ptr(), tc.data_ptr()],
             [B * H, ext.ELT_TANH], []),
            binary(ext.ELT_MUL, gate(s, 3), 4 * H, tc.data_ptr(), H,
                   h_un[t].data_ptr())]

    limit = ext.lstm_resident_max_h()
    plans, capture_ms = {}, {}
    for name in (["resident"] if H <= limit else []) + ["stepped"]:
        ext.set_lstm_resident_max_h(limit if name == "resident" else 0)
        plans[name], capture_ms[name] = _capture(fused(hs[name]), stream)
    ext.set_lstm_resident_max_h(-1)
    plans["unfused"], capture_ms["unfused"] = _capture(calls, stream)
    res = _alternate(plans, stream, rounds)
    torch.cuda.synchronize()
    out = {"B": B, "H": H, "T": T}
    for name, r in res.items():
        out[name] = {"us_per_step": round(r["median_us"] / T, 3),
                     "min": round(r["min_us"] / T, 3),
                     "max": round(r["max_us"] / T, 3),
                     "replays": r["replays"],
                     "capture_ms": round(capture_ms[name], 2)}
    ref = hs["stepped"].float()
    out["max_abs_diff_vs_stepped"] = {
        n: float((hs[n].float() - ref).abs().max()) for n in plans
        if n != "stepped"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_probe needs a GPU")
    stream = torch.cuda.Stream()
    out = [{"resident_max_h": ext.lstm_resident_max_h()}]
    print(json.dumps(out[0]), flush=True)
    for H in (64, 128, 256, 512, 1024):
        for B in (1, 8, 32):
            out.append(case(B, H, stream, args.rounds))
            print(json.dumps(out[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

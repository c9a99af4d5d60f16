#!/usr/bin/env python
"""Time K_LAYERNORM alone (profiles/memory_kernels_oracle.md).

    python scripts/layernorm_probe.py [path/to/_tfsc_engine*.so]

Without an argument the package's own extension is timed; with one, the
extension at that path (for instance a build of another commit), so two
builds can be alternated in one session. Per shape: one ExecPlan of 100
launches, warmed once, timed 7 times with device events; prints the
median, minimum and maximum in microseconds per launch.
"""
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

SHAPES = [(1024, 768), (16384, 768), (4096, 1024), (16384, 64)]
LAUNCHES, REPEATS = 100, 7


def load_ext(path):
    if path is None:
        from tfservingcache_amd.engine import _tfsc_engine as ext
        return ext
    spec = importlib.util.spec_from_file_location("_tfsc_engine", path)
    ext = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ext)
    return ext


def main():
    ext = load_ext(sys.argv[1] if len(sys.argv) > 1 else None)
    for rows, cols in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(rows, cols, generator=g).to(torch.bfloat16).cuda()
        gamma = torch.randn(cols, generator=g).to(torch.bfloat16).cuda()
        beta = torch.randn(cols, generator=g).to(torch.bfloat16).cuda()
        y = torch.empty_like(x)
        call = (ext.K_LAYERNORM, [x.data_ptr(), gamma.data_ptr(),
                                  beta.data_ptr(), y.data_ptr()],
                [rows, cols], [1e-12])
        plan = ext.ExecPlan([call] * LAUNCHES)
        plan.run()
        torch.cuda.synchronize()
        us = []
        for _ in range(REPEATS):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            plan.run()
            t1.record()
            torch.cuda.synchronize()
            us.append(t0.elapsed_time(t1) * 1000.0 / LAUNCHES)
        print(f"layernorm [{rows},{cols}]: median "
              f"{statistics.median(us):.2f} us/launch "
              f"(min {min(us):.2f}, max {max(us):.2f})", flush=True)


if __name__ == "__main__":
    main()

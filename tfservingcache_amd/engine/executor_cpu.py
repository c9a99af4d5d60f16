"""CPU reference executor — numpy fp32 interpretation of a Plan.

Serves three purposes:
  * serving fallback when no GPU is present (tests, config #1 half_plus_two
    on CPU — BASELINE.json configs[0]);
  * ground truth for the HIP engine's numerics tests (tests compare each
    CDNA4 kernel against this fp32 path);
  * documentation of each plan op's exact semantics.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from .planner import Plan, PlanOp, conv3d_transpose_phases, lstm_unpack


def _act(x: np.ndarray, act: str) -> np.ndarray:
    if act == "none":
        return x
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "relu6":
        return np.clip(x, 0.0, 6.0)
    if act == "tanh":
        return np.tanh(x)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if act == "gelu":
        from scipy.special import erf
        return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))
    raise ValueError(f"unknown act {act}")


_UNARY = {
    "relu": lambda x: np.maximum(x, 0.0),
    "relu6": lambda x: np.clip(x, 0.0, 6.0),
    "tanh": np.tanh,
    "sigmoid": lambda x: 1.0 / (1.0 + np.exp(-x)),
    "erf": None,  # filled lazily from scipy
    "sqrt": np.sqrt,
    "rsqrt": lambda x: 1.0 / np.sqrt(x),
    "exp": np.exp,
    "neg": np.negative,
    "square": np.square,
}

_BINARY = {
    "add": np.add, "sub": np.subtract, "mul": np.multiply,
    "div": np.divide, "max": np.maximum, "min": np.minimum,
    "sqdiff": lambda a, b: (a - b) ** 2,
}


def _resize_scale(n_in: int, n_out: int, align_corners: bool) -> np.float32:
    if align_corners and n_out > 1:
        return np.float32(n_in - 1) / np.float32(n_out - 1)
    return np.float32(n_in) / np.float32(n_out)


def _resize_nearest_idx(n_in, n_out, align_corners, half_pixel):
    """Source index per output index along one axis (TF
    ResizeNearestNeighbor), coordinates in f32."""
    d = np.arange(n_out, dtype=np.float32)
    scale = _resize_scale(n_in, n_out, align_corners)
    src = (d + np.float32(0.5)) * scale if half_pixel else d * scale
    fl = np.floor(src)
    if align_corners:
        # roundf: halves away from zero (src >= 0; src - fl is exact)
        fl = fl + (src - fl >= np.float32(0.5))
    return np.clip(fl.astype(np.int64), 0, n_in - 1)


def _resize_bilinear_coords(n_in, n_out, align_corners, half_pixel):
    """(lo, hi, lerp) per output index along one axis (TF
    ResizeBilinear), coordinates in f32."""
    d = np.arange(n_out, dtype=np.float32)
    scale = _resize_scale(n_in, n_out, align_corners)
    if half_pixel:
        src = (d + np.float32(0.5)) * scale - np.float32(0.5)
    else:
        src = d * scale
    fl = np.floor(src)
    lo = np.clip(fl.astype(np.int64), 0, n_in - 1)
    hi = np.clip(np.ceil(src).astype(np.int64), 0, n_in - 1)
    return lo, hi, (src - fl).astype(np.float32)


def _resize(x, out_hw, mode, align_corners, half_pixel):
    """NHWC image resize, f32. Bilinear interpolates along x, then y."""
    _, H, W, _ = x.shape
    Ho, Wo = out_hw
    if mode == "nearest":
        iy = _resize_nearest_idx(H, Ho, align_corners, half_pixel)
        ix = _resize_nearest_idx(W, Wo, align_corners, half_pixel)
        return np.ascontiguousarray(x[:, iy][:, :, ix], dtype=np.float32)
    y0, y1, ly = _resize_bilinear_coords(H, Ho, align_corners, half_pixel)
    x0, x1, lx = _resize_bilinear_coords(W, Wo, align_corners, half_pixel)
    lx = lx[None, None, :, None]
    ly = ly[None, :, None, None]
    rows0, rows1 = x[:, y0], x[:, y1]
    top = rows0[:, :, x0] + (rows0[:, :, x1] - rows0[:, :, x0]) * lx
    bot = rows1[:, :, x0] + (rows1[:, :, x1] - rows1[:, :, x0]) * lx
    return (top + (bot - top) * ly).astype(np.float32)


def combined_nms(boxes, scores, per_class, max_total, iou_thr, score_thr,
                 clip=True):
    """TF CombinedNonMaxSuppression with the tie order pinned. boxes
    [B,N,q,4] (q = 1 or C, rows y1,x1,y2,x2), scores [B,N,C]; `per_class`
    is P = min(max_output_size_per_class, N) and `max_total` the output
    rows M. Returns (boxes [B,M,4], scores [B,M], classes [B,M], all f32,
    valid [B] i32), rows past the valid count zero.

    Per image and class the boxes with score > score_thr (NaN fails) are
    visited by descending score, equal scores by lower box index; one is
    kept unless its IoU with an already kept box of the class is >
    iou_thr, until P are kept. IoU is TF's CPU kernel's, in f32: corners
    min/max-normalised, area <= 0 gives 0, else inter / (a_i + a_j -
    inter). The image's kept (class, box) pairs, by descending score, then
    lower class, then earlier kept, give the first M rows; the box leaves
    as given, clipped to [0, 1] when `clip`."""
    boxes = np.asarray(boxes, np.float32)
    scores = np.asarray(scores, np.float32)
    nb, n, c = scores.shape
    q = boxes.shape[2]
    f32 = np.float32
    lo = np.minimum(boxes[..., :2], boxes[..., 2:])
    hi = np.maximum(boxes[..., :2], boxes[..., 2:])
    area = (hi[..., 0] - lo[..., 0]) * (hi[..., 1] - lo[..., 1])
    out_b = np.zeros((nb, max_total, 4), f32)
    out_s = np.zeros((nb, max_total), f32)
    out_c = np.zeros((nb, max_total), f32)
    valid = np.zeros((nb,), np.int32)
    for b in range(nb):
        kept = []                        # (-score, class, rank, box index)
        for cl in range(c):
            qi = 0 if q == 1 else cl
            s = scores[b, :, cl]
            live = np.flatnonzero(s > f32(score_thr))
            live = live[np.argsort(-s[live], kind="stable")]
            rank = 0
            while live.size and rank < per_class:
                i, live = live[0], live[1:]
                kept.append((-s[i], cl, rank, i))
                rank += 1
                wh = np.maximum(
                    np.minimum(hi[b, i, qi], hi[b, live, qi]) -
                    np.maximum(lo[b, i, qi], lo[b, live, qi]), f32(0))
                inter = wh[:, 0] * wh[:, 1]
                ok = (area[b, i, qi] > 0) & (area[b, live, qi] > 0) & \
                    (inter > 0)
                union = area[b, i, qi] + area[b, live, qi] - inter
                iou = np.where(ok, inter / np.where(ok, union, f32(1)),
                               f32(0))
                live = live[~(iou > f32(iou_thr))]
        kept.sort()
        kept = kept[:max_total]
        valid[b] = len(kept)
        for m_, (ns, cl, _rank, i) in enumerate(kept):
            out_b[b, m_] = boxes[b, i, 0 if q == 1 else cl]
            out_s[b, m_] = -ns
            out_c[b, m_] = cl
    if clip:
        out_b = np.clip(out_b, f32(0), f32(1))
    return out_b, out_s, out_c, valid


class CpuExecutor:
    def __init__(self, plan: Plan):
        self.plan = plan

    def run(self, feeds: Dict[int, np.ndarray], batch: int,
            fetch: Optional[List[int]] = None) -> Dict[int, np.ndarray]:
        plan = self.plan
        vals: Dict[int, np.ndarray] = {}
        for t in plan.tensors:
            if t.kind == "weight" and t.weight is not None:
                vals[t.idx] = t.weight
        for idx, arr in feeds.items():
            if hasattr(arr, "materialize"):
                arr = arr.materialize()
            want = np.int32 if plan.tensors[idx].dtype == "i32" else np.float32
            vals[idx] = np.asarray(arr, dtype=want)
        # resolve aliases of fed tensors lazily below via _get

        def _get(i: int) -> np.ndarray:
            t = plan.tensors[i]
            if i in vals:
                return vals[i]
            if t.alias_of is not None:
                src = _get(t.alias_of)
                shape = plan.resolve_shape(t.shape, batch)
                vals[i] = src.reshape(shape)
                return vals[i]
            raise KeyError(f"tensor {i} ({t.name}) has no value")

        for op in plan.ops:
            self._run_op(op, _get, vals, batch)

        wanted = fetch if fetch is not None else list(plan.sig_outputs.values())
        return {i: _get(i) for i in wanted}

    # -- op semantics ------------------------------------------------------
    def _run_op(self, op: PlanOp, _get, vals, batch: int) -> None:
        k = op.kind
        p = op.params
        if k == "eltwise":
            fn = p["fn"]
            if len(op.inputs) == 1:
                f = _UNARY[fn]
                if fn == "erf":
                    from scipy.special import erf as _erf
                    f = _erf
                vals[op.outputs[0]] = f(_get(op.inputs[0])).astype(np.float32)
            else:
                a, b = _get(op.inputs[0]), _get(op.inputs[1])
                vals[op.outputs[0]] = _BINARY[fn](a, b).astype(np.float32)
        elif k == "gemm":
            a = _get(op.inputs[0])
            w = _get(op.inputs[1])
            if p.get("trans_a"):
                a = a.T
            if p.get("trans_b"):
                w = w.T
            y = a @ w
            ni = 2
            if p.get("has_bias"):
                y = y + _get(op.inputs[ni])
                ni += 1
            if p.get("residual"):
                y = y + _get(op.inputs[ni])
            y = _act(y, p.get("act", "none")).astype(np.float32)
            out_shape = self.plan.resolve_shape(
                self.plan.tensors[op.outputs[0]].shape, batch)
            vals[op.outputs[0]] = y.reshape(out_shape)
        elif k == "batched_gemm":
            a, b = _get(op.inputs[0]), _get(op.inputs[1])
            if p.get("trans_a"):
                a = np.swapaxes(a, -1, -2)
            if p.get("trans_b"):
                b = np.swapaxes(b, -1, -2)
            vals[op.outputs[0]] = (a @ b).astype(np.float32)
        elif k == "conv2d":
            self._conv2d(op, _get, vals)
        elif k == "depthwise_conv":
            self._depthwise(op, _get, vals)
        elif k == "pool":
            self._pool(op, _get, vals)
        elif k == "conv3d":
            self._conv3d(op, _get, vals)
        elif k == "pool3d":
            self._pool3d(op, _get, vals)
        elif k == "conv3d_transpose":
            self._conv3d_transpose(op, _get, vals)
        elif k == "lstm":
            self._lstm(op, _get, vals)
        elif k == "global_mean":
            x = _get(op.inputs[0])
            y = x.mean(axis=(1, 2), keepdims=p.get("keep", False))
            vals[op.outputs[0]] = y.astype(np.float32)
        elif k == "reduce_mean_mid":
            x = _get(op.inputs[0])
            y = x.mean(axis=1, keepdims=p.get("keep", False))
            vals[op.outputs[0]] = y.astype(np.float32)
        elif k == "reduce_mean_last":
            x = _get(op.inputs[0])
            y = x.mean(axis=-1, keepdims=p.get("keep", False))
            vals[op.outputs[0]] = y.astype(np.float32)
        elif k == "reduce":
            # the middle axis of the [outer, red, inner] view
            x = _get(op.inputs[0])
            f = {"mean": np.mean, "sum": np.sum, "max": np.max,
                 "min": np.min, "prod": np.prod}[p["fn"]]
            y = f(x.reshape(self.plan.resolve_shape(p["view"], batch)),
                  axis=1)
            out_shape = self.plan.resolve_shape(
                self.plan.tensors[op.outputs[0]].shape, batch)
            vals[op.outputs[0]] = y.astype(np.float32).reshape(out_shape)
        elif k == "softmax":
            x = _get(op.inputs[0])
            mx =x.max(axis=-1, keepdims=True)
            e = np.exp(x - mx)
            vals[op.outputs[0]] = (e / e.sum(axis=-1, keepdims=True)).astype(
                np.float32)
        elif k == "layernorm":
            x = _get(op.inputs[0])
            gamma = _get(op.inputs[1])
            beta = _get(op.inputs[2])
            mean = x.mean(axis=-1, keepdims=True)
            var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
            y = (x - mean) / np.sqrt(var + p["eps"]) * gamma + beta
            vals[op.outputs[0]] = y.astype(np.float32)
        elif k == "bn_act":
            x = _get(op.inputs[0])
            scale = _get(op.inputs[1])
            shift = _get(op.inputs[2])
            vals[op.outputs[0]] = _act(x * scale + shift,
                                       p.get("act", "none")).astype(np.float32)
        elif k == "pad":
            x = _get(op.inputs[0])
            pads = [(int(lo), int(hi)) for lo, hi in p["pads"]]
            vals[op.outputs[0]] = np.pad(x, pads).astype(np.float32)
        elif k == "transpose":
            x = _get(op.inputs[0])
            vals[op.outputs[0]] = np.transpose(x, p["perm"]).copy()
        elif k == "gather":
            table = _get(op.inputs[0])
            idx = _get(op.inputs[1]).astype(np.int64)
            vals[op.outputs[0]] = table[idx].astype(np.float32)
        elif k == "attention":
            q = _get(op.inputs[0])      # [B, S, H, D]
            kk_ = _get(op.inputs[1])
            v = _get(op.inputs[2])
            scale = p["scale"]
            scores = np.einsum("bqhd,bkhd->bhqk", q, kk_) * scale
            if len(op.inputs) > 3:
                bias = _get(op.inputs[3])
                bias = bias.reshape((1,) * (4 - bias.ndim) + bias.shape)
                scores = scores + np.broadcast_to(bias, scores.shape)
            mx = scores.max(-1, keepdims=True)
            # -inf biases: a fully masked row has max -inf; keep the
            # subtraction finite and let the row come out as zeros
            mx = np.where(np.isfinite(mx), mx, 0.0)
            e = np.exp(scores - mx)
            den = e.sum(-1, keepdims=True)
            probs = e / np.where(den > 0, den, 1.0)
            ctx = np.einsum("bhqk,bkhd->bqhd", probs, v)
            vals[op.outputs[0]] = ctx.astype(np.float32)
        elif k == "concat":
            parts = [_get(i) for i in op.inputs]
            vals[op.outputs[0]] = np.concatenate(parts, axis=p["axis"])
        elif k == "strided_copy":
            x = _get(op.inputs[0])
            sl = []
            for d in range(x.ndim):
                b = p["starts"][d]
                st = p["steps"][d]
                if p["shrink"][d]:
                    sl.append(b)
                else:
                    sl.append(slice(b, None, st))
            y = x[tuple(sl)]
            out_shape = self.plan.resolve_shape(
                self.plan.tensors[op.outputs[0]].shape, batch)
            vals[op.outputs[0]] = np.ascontiguousarray(
                y)[tuple(slice(0, dd) for dd in out_shape)].copy()
        elif k == "cast":
            x = _get(op.inputs[0])
            if p["mode"] == "i2f":
                vals[op.outputs[0]] = x.astype(np.float32)
            else:
                vals[op.outputs[0]] = x.astype(np.int32)
        elif k == "argmax_last":
            x = _get(op.inputs[0])
            vals[op.outputs[0]] = x.argmax(axis=-1).astype(np.int32)
        elif k == "topk_last":
            # TF TopKV2: values descending, equal values by lower index
            # (-0.0 == +0.0); the stable sort of -x is that order
            x = _get(op.inputs[0])
            idx = np.argsort(-x, axis=-1, kind="stable")[..., :p["k"]]
            vals[op.outputs[0]] = np.take_along_axis(x, idx, axis=-1)
            vals[op.outputs[1]] = idx.astype(np.int32)
        elif k == "combined_nms":
            res = combined_nms(_get(op.inputs[0]), _get(op.inputs[1]),
                               p["per_class"], p["max_total"], p["iou_thr"],
                               p["score_thr"], p["clip"])
            for o, v in zip(op.outputs, res):
                vals[o] = v
        elif k == "resize":
            vals[op.outputs[0]] = _resize(
                _get(op.inputs[0]), p["out_hw"], p["mode"],
                p["align_corners"], p["half_pixel_centers"])
        elif k == "zero_insert":
            x = _get(op.inputs[0])          # [N,h,w,C]
            sh, sw = p["stride"]
            Hz, Wz = p["out_hw"]
            z = np.zeros((x.shape[0], Hz, Wz, x.shape[3]), dtype=np.float32)
            z[:, ::sh, ::sw, :] = x
            vals[op.outputs[0]] = z
        else:
            raise ValueError(f"unknown plan op {k}")

    def _lstm(self, op: PlanOp, _get, vals) -> None:
        """The lstm op from its packed master weights (planner.lstm_pack),
        gates (i, ci, f, o); see planner.lower_lstm for the inputs."""
        p = op.params
        H = p["H"]
        sig = _UNARY["sigmoid"]
        x = _get(op.inputs[0])
        if p["x_batch_major"]:
            x = x.transpose(1, 0, 2)                     # -> [T,B,I]
        wx, wh, b = (_get(i) for i in op.inputs[1:4])
        ni = 4
        wci = wcf = wco = np.zeros(H, np.float32)
        if p["peephole"]:
            wci, wcf, wco = (_get(i) for i in op.inputs[4:7])
            ni = 7
        T, Bn = x.shape[:2]
        h = c = np.zeros((Bn, H), np.float32)
        if p["h0"]:
            h = _get(op.inputs[ni])
            ni += 1
        if p["c0"]:
            c = _get(op.inputs[ni])
        pre = lstm_unpack(x @ wx + b, H)                 # [T,B,4,H]
        whu = lstm_unpack(wh, H)                         # [H,4,H]
        hs = np.empty((T, Bn, H), np.float32)
        cs = np.empty((T, Bn, H), np.float32)
        for t in range(T):
            z = pre[t] + np.einsum("bk,kgj->bgj", h, whu)
            i = sig(z[:, 0] + c * wci)
            f = sig(z[:, 2] + c * wcf)
            c = np.tanh(z[:, 1]) * i + c * f
            if p["cell_clip"] > 0:
                c = np.clip(c, -p["cell_clip"], p["cell_clip"])
            h = sig(z[:, 3] + c * wco) * np.tanh(c)
            hs[t], cs[t] = h, c
        vals[op.outputs[0]] = hs.transpose(1, 0, 2).copy() \
            if p["h_batch_major"] else hs
        if p["cs"]:
            vals[op.outputs[1]] = cs

    def _conv2d(self, op: PlanOp, _get, vals) -> None:
        x = _get(op.inputs[0])          # [N,H,W,C]
        w = _get(op.inputs[1])          # [R,S,C,K]
        b = _get(op.inputs[2])          # [K]
        p = op.params
        sh, sw = p["stride"]
        pt, pb, pl, pr = p["pads"]
        R, S, C, K = w.shape
        N = x.shape[0]
        Ho, Wo = p["out_hw"]
        xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
        G = p.get("groups", 1)
        dh, dw = p.get("dilation", (1, 1))    # dense convs only
        if G == 1:
            # im2col; tap (r, s) starts at (r*dh, s*dw)
            cols = np.empty((N, Ho, Wo, R * S * C), dtype=np.float32)
            for r in range(R):
                for s in range(S):
                    patch = xp[:, r * dh:r * dh + sh * Ho:sh,
                               s * dw:s * dw + sw * Wo:sw, :]
                    cols[..., (r * S + s) * C:(r * S + s + 1) * C] = patch
            y = cols.reshape(-1, R * S * C) @ w.reshape(-1, K)
        else:
            # grouped: w is [R,S,Cg,K]; group g reads input channels
            # g*Cg.. and writes output channels g*Ng..
            Ng = K // G
            ys = []
            for gi in range(G):
                cols = np.empty((N, Ho, Wo, R * S * C), dtype=np.float32)
                for r in range(R):
                    for s in range(S):
                        patch = xp[:, r:r + sh * Ho:sh, s:s + sw * Wo:sw,
                                   gi * C:(gi + 1) * C]
                        cols[..., (r * S + s) * C:(r * S + s + 1) * C] = \
                            patch
                ys.append(cols.reshape(-1, R * S * C) @
                          w[..., gi * Ng:(gi + 1) * Ng].reshape(-1, Ng))
            y = np.concatenate(ys, axis=1)
        y = y.reshape(N, Ho, Wo, K) + b
        ni = 3
        if p.get("residual"):
            y = y + _get(op.inputs[ni])
        vals[op.outputs[0]] = _act(y, p.get("act", "none")).astype(np.float32)

    def _depthwise(self, op: PlanOp, _get, vals) -> None:
        x = _get(op.inputs[0])          # [N,H,W,C]
        w = _get(op.inputs[1])          # [R,S,C*M], k = c*M + m
        b = _get(op.inputs[2])          # [C*M]
        p = op.params
        sh, sw = p["stride"]
        pt, pb, pl, pr = p["pads"]
        R, S, K = w.shape
        M = p.get("mult", 1)
        dh, dw = p.get("dilation", (1, 1))    # M == 1 only
        N = x.shape[0]
        Ho, Wo = p["out_hw"]
        xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
        y = np.zeros((N, Ho, Wo, K), dtype=np.float32)
        for r in range(R):
            for s_ in range(S):
                patch = xp[:, r * dh:r * dh + sh * Ho:sh,
                           s_ * dw:s_ * dw + sw * Wo:sw, :]
                if M > 1:
                    # each input channel feeds M consecutive outputs
                    patch = np.repeat(patch, M, axis=-1)
                y += patch * w[r, s_]
        y = y + b
        vals[op.outputs[0]] = _act(y, p.get("act", "none")).astype(
            np.float32)

    @staticmethod
    def _windows3d(xp, window, stride, out_dhw):
        """The strided [N,Do,Ho,Wo,C] view of the padded NDHWC volume xp
        under each tap (a, b, c) of the window, in (a, b, c) order."""
        (sd, sh, sw), (Do, Ho, Wo) = stride, out_dhw
        for a in range(window[0]):
            for b in range(window[1]):
                for c in range(window[2]):
                    yield xp[:, a:a + sd * Do:sd, b:b + sh * Ho:sh,
                             c:c + sw * Wo:sw, :]

    def _conv3d(self, op: PlanOp, _get, vals) -> None:
        x = _get(op.inputs[0])          # [N,D,H,W,C]
        w = _get(op.inputs[1])          # [T*R,S,C,K], k = ((t*R+r)*S+s)*C+c
        b = _get(op.inputs[2])          # [K]
        p = op.params
        T, R, S, C, K = p["trsck"]
        pf, pk, pt, pb, pl, pr = p["pads"]
        Do, Ho, Wo = p["out_dhw"]
        xp = np.pad(x, ((0, 0), (pf, pk), (pt, pb), (pl, pr), (0, 0)))
        # im2col, one tap at a time
        cols = np.empty((x.shape[0], Do, Ho, Wo, T * R * S * C),
                        dtype=np.float32)
        for i, patch in enumerate(self._windows3d(xp, (T, R, S), p["stride"],
                                                  p["out_dhw"])):
            cols[..., i * C:(i + 1) * C] = patch
        y = cols.reshape(-1, T * R * S * C) @ w.reshape(-1, K)
        y = y.reshape(x.shape[0], Do, Ho, Wo, K) + b
        if p.get("residual"):
            y = y + _get(op.inputs[3])
        vals[op.outputs[0]] = _act(y, p.get("act", "none")).astype(np.float32)

    def _conv3d_transpose(self, op: PlanOp, _get, vals) -> None:
        x = _get(op.inputs[0])          # [N,D,H,W,Ci]
        w = _get(op.inputs[1])          # [n_taps,1,Ci,Co], phase-major taps
        b = _get(op.inputs[2])          # [Co]
        p = op.params
        T, R, S, Ci, Co = p["trsck"]
        sd, sh, sw = p["stride"]
        N, D, H, W, _ = x.shape
        # the uncropped result: tap (t,r,s) of x[i,j,l] lands on
        # (i*sd + t, j*sh + r, l*sw + s); at least pad + out long per axis
        full = [max((n - 1) * st + k, lo + o) for n, st, k, lo, o in zip(
            (D, H, W), p["stride"], (T, R, S), p["pads"], p["out_dhw"])]
        yf = np.zeros((N, *full, Co), dtype=np.float32)
        for _phase, taps, first in conv3d_transpose_phases((T, R, S),
                                                           p["stride"]):
            for i, (t, r, s) in enumerate(taps):
                yf[:, t:t + (D - 1) * sd + 1:sd, r:r + (H - 1) * sh + 1:sh,
                   s:s + (W - 1) * sw + 1:sw, :] += x @ w[first + i, 0]
        (pf, pt, pl), (Do, Ho, Wo) = p["pads"], p["out_dhw"]
        y = yf[:, pf:pf + Do, pt:pt + Ho, pl:pl + Wo, :] + b
        if p.get("residual"):
            y = y + _get(op.inputs[3])
        vals[op.outputs[0]] = _act(y, p.get("act", "none")).astype(np.float32)

    def _pool3d(self, op: PlanOp, _get, vals) -> None:
        x = _get(op.inputs[0])          # [N,D,H,W,C]
        p = op.params
        pf, pk, pt, pb, pl, pr = p["pads"]
        pad = ((0, 0), (pf, pk), (pt, pb), (pl, pr), (0, 0))
        geom = (p["ksize"], p["stride"], p["out_dhw"])
        if p["mode"] == "max":
            xp = np.pad(x, pad, constant_values=-np.inf)
            out = np.maximum.reduce(list(self._windows3d(xp, *geom)))
        else:
            # padded cells are excluded from the divisor, as in _pool
            ones = np.pad(np.ones((1,) + x.shape[1:4] + (1,), np.float32),
                          pad)
            out = sum(self._windows3d(np.pad(x, pad), *geom)) / \
                np.maximum(sum(self._windows3d(ones, *geom)), 1.0)
        vals[op.outputs[0]] = out.astype(np.float32)

    def _pool(self, op: PlanOp, _get, vals) -> None:
        x = _get(op.inputs[0])
        p = op.params
        kh, kw = p["ksize"]
        sh, sw = p["stride"]
        pt, pb, pl, pr = p["pads"]
        Ho, Wo = p["out_hw"]
        if p["mode"] == "max":
            xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)),
                        constant_values=-np.inf)
        else:
            xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
        N, _, _, C = x.shape
        out = np.empty((N, Ho, Wo, C), dtype=np.float32)
        stack = np.empty((kh * kw, N, Ho, Wo, C), dtype=np.float32)
        for i in range(kh):
            for j in range(kw):
                stack[i * kw + j] = xp[:, i:i + sh * Ho:sh, j:j + sw * Wo:sw, :]
        if p["mode"] == "max":
            out = stack.max(axis=0)
        else:
            # TF AvgPool excludes padded cells from the divisor (the
            # GPU kernels count valid cells the same way)
            ones = np.pad(np.ones((1, x.shape[1], x.shape[2], 1),
                                  dtype=np.float32),
                          ((0, 0), (pt, pb), (pl, pr), (0, 0)))
            cnt = np.zeros((1, Ho, Wo, 1), dtype=np.float32)
            for i in range(kh):
                for j in range(kw):
                    cnt += ones[:, i:i + sh * Ho:sh, j:j + sw * Wo:sw, :]
            out = stack.sum(axis=0) / np.maximum(cnt, 1.0)
        vals[op.outputs[0]] = out

#!/usr/bin/env python3
"""Flagship serving benchmark — the driver contract.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
                    [--full]

Measures the BASELINE.json headline: predict req/sec (whole node) plus
p50 cold-load latency. A plain run does only what that figure needs:
set up, warm up, time the K steps, print one JSON result line. --full
adds the secondary measurements that take runs of their own (today:
the headline's warm-cache req/sec half). --dump-outputs DIR writes the
responses of the last timed step as DIR/<output name>.npy (one row per
request, in request order) so two builds can be compared output for
output; inputs and the request schedule are seeded. One rank per GPU (the driver launches ranks via
torch.distributed.run for N>1); each rank runs the full node-local
serving stack — disk model repo -> DiskModelProvider -> byte-budget LRU
-> GPU model pool (CDNA4 HIP engine, bf16) — and drives it with
concurrent Predict requests through the gRPC message path (protobuf
decode -> CacheManager -> engine -> protobuf encode; TCP loopback
excluded). A "step" is REQS_PER_STEP completed requests per rank.

Modes (--mode):
  headline  (default) the BASELINE.json headline workload: 1000
        hardlinked ResNet-50 models, per-GPU pool capped at 10, Zipf-1.1
        access, served over the NATIVE socket front-end (real gRPC over
        TCP loopback). Emits BOTH metric halves: LRU predict req/sec
        (the timed region) and p50 cold-load latency; with --full also
        a warm-cache req/sec measured separately BEFORE the timed
        region. With world>1 it becomes the ring workload
        (configs[3]): ownership by
        consistent hash over ranks, replicas=2, replica fan-out over
        the RCCL/xGMI plane at preload.
  warm  ResNet-50 warm-cache predict loop (BASELINE configs[1])
  lru   --models N ResNet-50s, pool capped at --pool-size, Zipf access:
        the evict/reload path (BASELINE configs[2]); cold-load latencies
        recorded from the pool.
  ring  consistent-hash ring over the N ranks/GPUs with
        --replicas replicas per model; model files fan out to replica
        GPUs over the RCCL/xGMI replica plane at preload; each rank
        serves Zipf-weighted requests for the models it owns
        (BASELINE configs[3]/[4]). --model mixed serves BERT-base +
        ResNet-50 together (configs[4]).

Data: synthetic (random normal images), random-init weights — no
network/datasets in this environment; stated in the "data" field.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tfservingcache_amd.cachemanager import (CacheManager, LRUCache,  # noqa: E402
                                             ModelPool, make_cpu_loader,
                                             make_gpu_loader)
from tfservingcache_amd.cachemanager.providers import DiskModelProvider  # noqa: E402
from tfservingcache_amd.models.builders import (build_resnet50,  # noqa: E402
                                                build_bert,
                                                build_mobilenet_v2)
from tfservingcache_amd.engine.savedmodel import write_saved_model  # noqa: E402
from tfservingcache_amd.tfservingproxy import LocalServingHandler  # noqa: E402
from tfservingcache_amd.wire import messages as m  # noqa: E402
from tfservingcache_amd.wire.tensor import numpy_to_tensorproto  # noqa: E402

REQS_PER_STEP = 100


def _client_proc_main(conn, port, model_name, model_kind, batch,
                      image_size, seq_len, threads, channels,
                      transport="native"):
    """Spawned client worker (warm mode): builds its own request bytes,
    opens its own channels/sockets, executes 'run N' commands from the
    parent over the pipe, returns per-request latencies."""
    import numpy as _np
    import time as _time
    from concurrent.futures import ThreadPoolExecutor as _TPE

    rng = _np.random.default_rng(os.getpid())

    if transport == "native-rest":
        import json as _json
        import socket as _socket
        import threading as _threading
        if model_kind == "bert_base":
            payload = {"instances": rng.integers(
                0, 30000, (batch, seq_len)).astype(int).tolist()}
        else:
            payload = {"instances": _np.round(
                rng.standard_normal(
                    (batch, image_size, image_size, 3)) * 0.5,
                5).tolist()}
        body = _json.dumps(payload).encode()
        raw = (f"POST /v1/models/{model_name}:predict HTTP/1.1\r\n"
               f"Host: 127.0.0.1\r\n"
               f"Content-Type: application/json\r\n"
               f"Content-Length: {len(body)}\r\n\r\n"
               ).encode() + body
        tl = _threading.local()

        def one(i):
            t0 = _time.monotonic()
            sock = getattr(tl, "sock", None)
            if sock is None:
                sock = _socket.create_connection(("127.0.0.1", port),
                                                 timeout=300)
                sock.setsockopt(_socket.IPPROTO_TCP,
                                _socket.TCP_NODELAY, 1)
                tl.sock = sock
                tl.buf = b""
            sock.sendall(raw)
            buf = tl.buf
            while b"\r\n\r\n" not in buf:
                buf += sock.recv(1 << 16)
            head, rest = buf.split(b"\r\n\r\n", 1)
            clen = 0
            for line in head.split(b"\r\n"):
                if line.lower().startswith(b"content-length"):
                    clen = int(line.split(b":")[1])
            while len(rest) < clen:
                rest += sock.recv(1 << 18)
            tl.buf = rest[clen:]
            if not head.startswith(b"HTTP/1.1 200"):
                raise RuntimeError(head[:60].decode(errors="replace"))
            return _time.monotonic() - t0

        pool = _TPE(max_workers=threads)
        while True:
            cmd = conn.recv()
            if cmd[0] == "stop":
                conn.close()
                return
            _, n = cmd
            lats = list(pool.map(one, range(n)))
            conn.send(lats)
        return

    import grpc as grpc_mod
    from tfservingcache_amd.wire import messages as _m
    from tfservingcache_amd.wire.tensor import numpy_to_tensorproto as _n2t
    if model_kind == "bert_base":
        inputs = {"input_ids": _n2t(rng.integers(
            0, 30000, (batch, seq_len)).astype(_np.int32))}
    else:
        inputs = {"input": _n2t((rng.standard_normal(
            (batch, image_size, image_size, 3)) * 0.5
        ).astype(_np.float32))}
    req = _m.PredictRequest(
        model_spec=_m.ModelSpec(name=model_name,
                                version=_m.Int64Value(value=1)),
        inputs=inputs).encode()
    rpcs = []
    for ci in range(max(1, channels)):
        ch = grpc_mod.insecure_channel(
            f"127.0.0.1:{port}",
            options=[("grpc.max_receive_message_length", 256 << 20),
                     ("grpc.max_send_message_length", 256 << 20),
                     ("tfsc.channel_id", ci)])
        rpcs.append(ch.unary_unary(
            "/tensorflow.serving.PredictionService/Predict",
            request_serializer=lambda b: b,
            response_deserializer=lambda b: b))

    pool = _TPE(max_workers=threads)

    def one(i):
        t0 = _time.monotonic()
        rpcs[i % len(rpcs)](req, timeout=300)
        return _time.monotonic() - t0

    while True:
        cmd = conn.recv()
        if cmd[0] == "stop":
            conn.close()
            return
        _, n = cmd
        lats = list(pool.map(one, range(n)))
        conn.send(lats)


def _link_tree(src: str, dst: str) -> None:
    for root, _dirs, files in os.walk(src):
        rel = os.path.relpath(root, src)
        os.makedirs(os.path.join(dst, rel), exist_ok=True)
        for f in files:
            os.link(os.path.join(root, f), os.path.join(dst, rel, f))


def build_repo(base: str, n_models: int, image_size: int,
               model_kind: str = "resnet50", seq_len: int = 128) -> list:
    """Write one SavedModel per family, hard-link into n_models dirs.
    Returns [(name, kind)]."""
    kinds = (["resnet50", "bert_base"] if model_kind == "mixed"
             else [model_kind])
    protos = {}
    for kind in kinds:
        proto_dir = os.path.join(base, f"_proto_{kind}", "1")
        if kind == "resnet50":
            sm = build_resnet50(image_size=image_size, num_classes=1000)
        elif kind == "mobilenet_v2":
            sm = build_mobilenet_v2(image_size=image_size,
                                    num_classes=1000)
        else:
            sm = build_bert(seq_len=seq_len)
        write_saved_model(sm, proto_dir)
        protos[kind] = proto_dir
    names = []
    for i in range(n_models):
        kind = kinds[i % len(kinds)]
        name = f"{kind}_{i:04d}"
        _link_tree(protos[kind], os.path.join(base, name, "1"))
        names.append((name, kind))
    return names


def _start_s3_mock(repo: str):
    """In-process S3-compatible store over the generated repo: ListV2
    + streamed GETs served from disk. Cold loads then pay a real
    per-object HTTP download (the s3Provider regime of BASELINE
    configs[4]) instead of the disk provider's hardlink fetch."""
    import http.server
    import urllib.parse
    from tfservingcache_amd.cachemanager.providers.s3 import \
        S3ModelProvider

    index = {}
    for root, _dirs, files in os.walk(repo):
        for f in files:
            full = os.path.join(root, f)
            key = os.path.relpath(full, repo).replace(os.sep, "/")
            index[key] = full
    keys_sorted = sorted(index)

    class Handler(http.server.BaseHTTPRequestHandler):
        protocol_version = "HTTP/1.1"

        def log_message(self, *a):      # noqa: N802
            pass

        def do_GET(self):               # noqa: N802
            parsed = urllib.parse.urlparse(self.path)
            qs = dict(urllib.parse.parse_qsl(parsed.query))
            if qs.get("list-type") == "2":
                prefix = qs.get("prefix", "")
                body = ['<?xml version="1.0"?><ListBucketResult>']
                import bisect
                i = bisect.bisect_left(keys_sorted, prefix)
                while i < len(keys_sorted) and \
                        keys_sorted[i].startswith(prefix):
                    k = keys_sorted[i]
                    body.append(
                        f"<Contents><Key>{k}</Key>"
                        f"<Size>{os.path.getsize(index[k])}</Size>"
                        f"</Contents>")
                    i += 1
                body.append("<IsTruncated>false</IsTruncated>"
                            "</ListBucketResult>")
                data = "".join(body).encode()
                self.send_response(200)
                self.send_header("Content-Length", str(len(data)))
                self.end_headers()
                self.wfile.write(data)
                return
            path = urllib.parse.unquote(parsed.path).lstrip("/")
            _bucket, _, key = path.partition("/")
            full = index.get(key)
            if full is None:
                self.send_response(404)
                self.send_header("Content-Length", "0")
                self.end_headers()
                return
            size = os.path.getsize(full)
            self.send_response(200)
            self.send_header("Content-Length", str(size))
            self.end_headers()
            with open(full, "rb") as f:
                while True:
                    chunk = f.read(1 << 20)
                    if not chunk:
                        break
                    self.wfile.write(chunk)

    srv = http.server.ThreadingHTTPServer(("127.0.0.1", 0), Handler)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    return S3ModelProvider(
        bucket="models", base_path="",
        endpoint_url=f"http://127.0.0.1:{srv.server_address[1]}")


def _graph_status(pool):
    try:
        for e in pool._entries.values():      # noqa: SLF001
            gm = getattr(e.model, "_gpu", None)
            if gm is not None and gm._contexts:  # noqa: SLF001
                ctxs = [c for lst in gm._contexts.values() for c in lst]
                return bool(ctxs) and all(
                    c.captured and c.exec_plan.has_graph() for c in ctxs)
    except Exception:       # noqa: BLE001
        pass
    return None


DUMP_BYTES_MAX = 64 * 1000 * 1000


def _dump_outputs(out_dir, captured, transport, rank, world) -> None:
    """Write the captured responses of the last timed step: one
    DIR/<output name>.npy per response tensor, rows in request order.
    Rank r>0 of a multi-rank run writes <output name>.rank<r>.npy."""
    from tfservingcache_amd.wire.tensor import tensorproto_to_numpy
    per_name = {}
    for i in sorted(captured):
        resp = captured[i]
        if transport == "native-rest":
            body = json.loads(resp)
            if "predictions" in body:
                outs = {"predictions": np.asarray(body["predictions"])}
            else:
                outs = body["outputs"]
                if not isinstance(outs, dict):
                    outs = {"outputs": outs}
                outs = {k: np.asarray(v) for k, v in outs.items()}
        else:
            if isinstance(resp, (bytes, bytearray, memoryview)):
                resp = m.PredictResponse.decode(bytes(resp))
            outs = {k: tensorproto_to_numpy(tp)
                    for k, tp in resp.outputs.items()}
        for k, v in outs.items():
            per_name.setdefault(k, []).append(v)
    if not per_name:
        raise SystemExit("--dump-outputs: the last timed step returned "
                         "no responses")
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_BYTES_MAX // len(per_name)
    for k in sorted(per_name):
        arr = np.stack(per_name[k])
        if arr.dtype != np.float64:
            arr = arr.astype(np.float32)
        if arr.nbytes > budget:
            # fixed, seeded sample of the flattened tensor
            idx = np.sort(np.random.default_rng(0).integers(
                0, arr.size, budget // arr.itemsize))
            arr = arr.reshape(-1)[idx]
        safe = "".join(c if c.isalnum() or c in "-_." else "_" for c in k)
        if world > 1 and rank > 0:
            safe += f".rank{rank}"
        np.save(os.path.join(out_dir, safe + ".npy"), arr)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode",
                    choices=["headline", "warm", "lru", "ring"],
                    default="headline")
    ap.add_argument("--model",
                    choices=["resnet50", "mobilenet_v2", "bert_base",
                             "mixed"],
                    default="resnet50")
    ap.add_argument("--replicas", type=int, default=2,
                    help="replicasPerModel (ring mode)")
    ap.add_argument("--seq-len", type=int, default=128,
                    help="BERT sequence length")
    ap.add_argument("--batch", type=int, default=None,
                    help="images per predict request "
                         "(default: 8 headline, 16 otherwise)")
    ap.add_argument("--models", type=int, default=None,
                    help="models in the repo (default: 1000 headline, "
                         "100 lru/ring)")
    ap.add_argument("--pool-size", type=int, default=10,
                    help="models resident per GPU (lru mode)")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--threads", type=int, default=10,
                    help="concurrent client threads per rank")
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--cpu", action="store_true",
                    help="CPU engine (CI smoke only; not a benchmark)")
    ap.add_argument("--dyn-batch", action="store_true",
                    help="enable server-side dynamic batching")
    ap.add_argument("--batch-timeout-ms", type=float, default=1.0,
                    help="dynamic-batching merge window")
    ap.add_argument("--provider", choices=["disk", "s3-mock"],
                    default="disk",
                    help="model store: local disk (hardlink fetch) or "
                         "an in-process S3-compatible HTTP server over "
                         "the same repo (real downloads per cold load "
                         "- BASELINE configs[4] s3Provider)")
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16",
                    help="engine compute dtype (fp8: e4m3 GEMMs with "
                         "rowwise dequant; conv stays bf16)")
    ap.add_argument("--streams", type=int, default=6,
                    help="execution contexts (HIP streams) per model")
    ap.add_argument("--channels", type=int, default=1,
                    help="client gRPC channels (grpc/native transports)")
    ap.add_argument("--client-procs", type=int, default=0,
                    help="run gRPC clients in N separate PROCESSES "
                         "(warm mode, grpc/native transports): measures "
                         "the server without the client's GIL in the "
                         "way")
    ap.add_argument("--transport",
                    choices=["inproc", "grpc", "native", "native-rest"],
                    default=None,
                    help="inproc: gRPC message path without sockets; "
                         "grpc: Python grpcio server over TCP loopback; "
                         "native: C++ nghttp2 gRPC front-end over TCP "
                         "loopback (registered Predicts bypass Python); "
                         "native-rest: C++ HTTP/1.1 JSON front-end over "
                         "TCP loopback")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements that need "
                         "runs of their own (headline: the warm-cache "
                         "req/sec half); off by default so a plain run "
                         "only times the headline steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the responses of "
                         "the LAST timed step as DIR/<output name>.npy "
                         "(float32/float64, one row per request in "
                         "request order; a fixed seeded sample when "
                         "over 64 MB in all)")
    args = ap.parse_args()
    if args.dump_outputs and args.client_procs > 0:
        raise SystemExit("--dump-outputs needs in-process clients "
                         "(drop --client-procs)")
    if args.dump_outputs and args.steps < 1:
        raise SystemExit("--dump-outputs needs at least one timed step")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    # headline = the BASELINE workload; resolves to the LRU-churn path
    # on one rank and the ring/replica path on many, over real sockets
    headline = args.mode == "headline"
    if args.batch is None:
        args.batch = 8 if headline else 16
    if args.models is None:
        args.models = 1000 if headline else 100
    if args.transport is None:
        args.transport = "native" if headline else "inproc"
    eff_mode = args.mode
    if headline:
        eff_mode = "lru" if world == 1 else "ring"

    dist = None
    torch = None
    if not args.cpu:
        import torch  # noqa: F811
    if world > 1:
        import torch  # noqa: F811
        import torch.distributed as dist  # noqa: F811
        backend = os.environ.get("TFSC_BENCH_BACKEND") or (
            "gloo" if (args.cpu or not torch.cuda.is_available())
            else "nccl")
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend)

    if args.cpu:
        device = "cpu"
    else:
        import torch as _t
        n_dev = max(_t.cuda.device_count(), 1)
        device = f"cuda:{local_rank % n_dev}"

    tmp = tempfile.mkdtemp(prefix=f"tfsc_bench_r{rank}_")
    repo = os.path.join(tmp, "repo")
    cache_dir = os.path.join(tmp, "cache")
    n_models = args.models if eff_mode in ("lru", "ring") else 1
    named = build_repo(repo, n_models, args.image_size, args.model,
                       args.seq_len)
    names = [n for n, _k in named]
    kind_of = dict(named)

    if args.provider == "s3-mock":
        provider = _start_s3_mock(repo)
    else:
        provider = DiskModelProvider(repo)
    cache = LRUCache(cache_dir, max_size_bytes=200 * 10 ** 9)
    pool_cap = args.pool_size if eff_mode in ("lru", "ring") else 4
    if args.cpu:
        loader = make_cpu_loader(cache)
    else:
        loader = make_gpu_loader(cache, device=device,
                                 max_batch=max(args.batch, 64)
                                 if args.dyn_batch else max(args.batch, 1),
                                 batching=args.dyn_batch,
                                 batch_timeout_s=args.batch_timeout_ms
                                 / 1e3,
                                 n_streams=args.streams,
                                 dtype=args.dtype,
                                 prewarm_batch=(args.batch
                                                if eff_mode in
                                                ("lru", "ring")
                                                else None))
    pool = ModelPool(loader, max_concurrent_models=pool_cap, device=device)
    cm = CacheManager(provider, cache, pool, model_fetch_timeout=300.0)
    handler = LocalServingHandler(cm)

    # pre-encoded request bytes (shared payloads; model name swapped)
    img = (np.random.default_rng(rank).standard_normal(
        (args.batch, args.image_size, args.image_size, 3)) * 0.5
    ).astype(np.float32)
    tp_img = numpy_to_tensorproto(img)
    ids = np.random.default_rng(rank).integers(
        0, 30000, (args.batch, args.seq_len)).astype(np.int32)
    tp_ids = numpy_to_tensorproto(ids)

    def request_bytes(name: str) -> bytes:
        if kind_of[name] == "bert_base":
            inputs = {"input_ids": tp_ids}
        else:
            inputs = {"input": tp_img}
        return m.PredictRequest(
            model_spec=m.ModelSpec(name=name, version=m.Int64Value(value=1)),
            inputs=inputs).encode()

    req_cache = {n: request_bytes(n) for n in names}

    rng = np.random.default_rng(1234 + rank)
    probs_all = 1.0 / np.arange(1, n_models + 1) ** args.zipf
    probs_all /= probs_all.sum()
    order = rng.permutation(n_models)

    warm_name = None
    if eff_mode == "ring":
        # ring over ranks; this rank serves the models it owns
        from tfservingcache_amd.taskhandler import (ConsistentHashRing,
                                                    model_key)
        from tfservingcache_amd.parallel import ReplicaPlane
        ring = ConsistentHashRing()
        ring.set_members([f"rank{r}" for r in range(world)])

        def owners_of(name, version=1):
            mems = ring.get_n(model_key(name, version),
                              min(args.replicas, world))
            return sorted(int(mm[4:]) for mm in mems)

        owned_idx = [i for i, n in enumerate(names)
                     if rank in owners_of(n)]
        if world > 1:
            # RCCL/xGMI fan-out of the model BYTES: rank 0 stages each
            # FAMILY prototype once and broadcasts it over the plane
            # (nccl == RCCL on GPU nodes); every rank then hardlinks its
            # owned models from the landed prototype — the same
            # content-dedup the hardlinked model repo already states in
            # the bench config. (Fanning out 1000 byte-identical copies
            # individually would move ~100 GB of duplicate bytes.)
            from tfservingcache_amd.cachemanager.lrucache import (
                Model as CacheModel, dir_size)
            plane = ReplicaPlane(device=device if not args.cpu else None)
            for kind in sorted(set(kind_of.values())):
                pname = f"_proto_{kind}"
                if rank == 0:
                    provider.load_model(pname, 1, cache.base_dir)
                vdir = os.path.join(cache.base_dir, pname, "1")
                plane.replicate_files(vdir, 0, list(range(world)))
                for i in owned_idx:
                    n = names[i]
                    if kind_of[n] != kind:
                        continue
                    dst = os.path.join(cache.base_dir, n, "1")
                    if not os.path.isdir(dst):
                        _link_tree(vdir, dst)
                    cache.put(CacheModel(name=n, version=1,
                                         path=os.path.join(n, "1"),
                                         size_on_disk=dir_size(dst)))
        if not owned_idx:
            owned_idx = [rank % n_models]
        w = probs_all[owned_idx]
        w = w / w.sum()
        owned_names = [names[i] for i in owned_idx]

        # precomputed schedule: Generator.choice is not thread-safe
        sched = rng.choice(np.arange(len(owned_names)), size=65536, p=w)

        def pick(i):
            return owned_names[sched[i % 65536]]
        warm_name = owned_names[0]
    elif eff_mode == "lru":
        sched = rng.choice(np.arange(n_models), size=65536, p=probs_all)

        def pick(i):
            return names[order[sched[i % 65536]]]
        warm_name = names[order[sched[0]]]
    else:
        def pick(i):
            return names[0]
        warm_name = names[0]

    lat_lock = threading.Lock()
    latencies = []          # per-request wall seconds (timed section)
    timing_on = [False]
    capture_on = [False]    # --dump-outputs: keep the last step's replies
    captured = {}           # request index -> raw response

    def timed(fn):
        def run(i):
            t0 = time.monotonic()
            resp = fn(i)
            if timing_on[0]:
                with lat_lock:
                    latencies.append(time.monotonic() - t0)
            if capture_on[0]:
                captured[i] = resp
        return run

    grpc_server = None
    if args.transport == "native-rest":
        import socket as socket_mod
        import threading as threading_mod
        from tfservingcache_amd.tfservingproxy.native_frontend import \
            NativeRestServer
        grpc_server = NativeRestServer(handler)
        grpc_server.add_insecure_port("127.0.0.1:0")
        grpc_server.start()
        rport = grpc_server.port

        def _on_avail_rest(name, version, model):
            fast = getattr(getattr(model, "_gpu", None), "_fast", None)
            if fast is not None:
                grpc_server.register_model(name, version, fast)
        pool.on_available = _on_avail_rest
        pool.on_unload = (lambda name, version, model:
                          grpc_server.unregister_model(name, version))

        # pre-encoded HTTP request bytes per model (one JSON body per
        # family; only the path differs)
        import json as json_mod
        bodies = {}

        def _rest_body(kind: str) -> bytes:
            if kind not in bodies:
                if kind == "bert_base":
                    payload = {"instances": ids.tolist()}
                else:
                    payload = {"instances": np.round(img, 5).tolist()}
                bodies[kind] = json_mod.dumps(payload).encode()
            return bodies[kind]

        rest_reqs = {}
        for n in names:
            body = _rest_body(kind_of[n])
            head = (f"POST /v1/models/{n}:predict HTTP/1.1\r\n"
                    f"Host: 127.0.0.1\r\n"
                    f"Content-Type: application/json\r\n"
                    f"Content-Length: {len(body)}\r\n\r\n"
                    ).encode()
            rest_reqs[n] = head + body

        tl = threading_mod.local()

        def _rest_call(name: str) -> bytes:
            sock = getattr(tl, "sock", None)
            if sock is None:
                sock = socket_mod.create_connection(
                    ("127.0.0.1", rport), timeout=300)
                sock.setsockopt(socket_mod.IPPROTO_TCP,
                                socket_mod.TCP_NODELAY, 1)
                tl.sock = sock
                tl.buf = b""
            sock.sendall(rest_reqs[name])
            buf = tl.buf
            while b"\r\n\r\n" not in buf:
                chunk = sock.recv(1 << 16)
                if not chunk:
                    raise RuntimeError("rest connection closed")
                buf += chunk
            head, rest = buf.split(b"\r\n\r\n", 1)
            status = int(head.split(b" ", 2)[1])
            clen = 0
            for line in head.split(b"\r\n"):
                if line.lower().startswith(b"content-length"):
                    clen = int(line.split(b":")[1])
            while len(rest) < clen:
                chunk = sock.recv(1 << 18)
                if not chunk:
                    raise RuntimeError("rest connection closed")
                rest += chunk
            tl.buf = rest[clen:]
            if status != 200:
                raise RuntimeError(
                    f"rest predict failed: {status} "
                    f"{rest[:200].decode(errors='replace')}")
            return rest[:clen]

        def one_request(i: int):
            return _rest_call(pick(i))
    elif args.transport in ("grpc", "native"):
        import grpc as grpc_mod
        if args.transport == "native":
            from tfservingcache_amd.tfservingproxy.native_frontend import \
                NativeGrpcServer
            grpc_server = NativeGrpcServer(
                handler, workers=max(args.threads, 8))
            grpc_server.add_insecure_port("127.0.0.1:0")
            grpc_server.start()
            gport = grpc_server.port
            # pool -> registry so warmed Predicts run fully in C++
            def _on_avail(name, version, model):
                fast = getattr(getattr(model, "_gpu", None), "_fast",
                               None)
                if fast is not None:
                    grpc_server.register_model(name, version, fast)
            pool.on_available = _on_avail
            pool.on_unload = (lambda name, version, model:
                              grpc_server.unregister_model(name, version))
        else:
            from tfservingcache_amd.tfservingproxy import \
                make_cache_grpc_server
            grpc_server, _health = make_cache_grpc_server(
                handler, max_workers=max(args.threads * 2, 8),
                max_msg=256 * 1024 * 1024)
            gport = grpc_server.add_insecure_port("127.0.0.1:0")
            grpc_server.start()
        rpcs = []
        for ci in range(max(1, args.channels)):
            channel = grpc_mod.insecure_channel(
                f"127.0.0.1:{gport}",
                options=[("grpc.max_receive_message_length",
                          256 * 1024 * 1024),
                         ("grpc.max_send_message_length",
                          256 * 1024 * 1024),
                         # distinct arg -> distinct subchannel per channel
                         ("tfsc.channel_id", ci)])
            rpcs.append(channel.unary_unary(
                "/tensorflow.serving.PredictionService/Predict",
                request_serializer=lambda b: b,
                response_deserializer=m.PredictResponse.decode))

        def one_request(i: int):
            return rpcs[i % len(rpcs)](req_cache[pick(i)], timeout=300)
    else:
        def one_request(i: int):
            return handler.predict_bytes(req_cache[pick(i)])

    one_request = timed(one_request)

    # initial load (timed -> cold-load sample even in warm mode)
    t0 = time.monotonic()
    one_request(0)
    first_load_s = time.monotonic() - t0

    pool_executor = ThreadPoolExecutor(max_workers=args.threads)

    # headline --full: measure the WARM-cache half first (one resident
    # model, same transport), strictly outside the LRU timed region
    warm_req_per_sec = None
    if headline and args.full:
        if args.transport == "native-rest":
            def warm_one(i: int) -> None:
                _rest_call(warm_name)
        elif args.transport in ("grpc", "native"):
            def warm_one(i: int) -> None:
                rpcs[i % len(rpcs)](req_cache[warm_name], timeout=300)
        else:
            def warm_one(i: int) -> None:
                handler.predict_bytes(req_cache[warm_name])
        warm_one(0)                       # ensure resident + contexts
        for _ in range(3):                # context warm-up passes
            list(pool_executor.map(warm_one, range(50)))
        wt0 = time.monotonic()
        wn = 0
        while time.monotonic() - wt0 < 2.0:
            list(pool_executor.map(warm_one, range(100)))
            wn += 100
        warm_req_per_sec = wn / (time.monotonic() - wt0)

    client_conns = []
    client_procs = []
    if args.client_procs > 0:
        if args.transport not in ("grpc", "native", "native-rest") or \
                eff_mode != "warm":
            raise SystemExit("--client-procs needs warm mode and a "
                             "socket transport")
        import multiprocessing as mp
        ctx = mp.get_context("spawn")
        per = max(1, args.threads // args.client_procs)
        for _ in range(args.client_procs):
            parent, child = ctx.Pipe()
            proc = ctx.Process(
                target=_client_proc_main,
                args=(child, gport if args.transport != "native-rest"
                      else rport,
                      names[0], kind_of[names[0]],
                      args.batch, args.image_size, args.seq_len, per,
                      max(1, args.channels // args.client_procs),
                      args.transport),
                daemon=True)
            proc.start()
            client_conns.append(parent)
            client_procs.append(proc)

    def step(base: int) -> None:
        if client_conns:
            n = REQS_PER_STEP // len(client_conns)
            extra = REQS_PER_STEP - n * len(client_conns)
            for i, conn in enumerate(client_conns):
                conn.send(("run", n + (extra if i == 0 else 0)))
            for conn in client_conns:
                lats = conn.recv()
                if timing_on[0]:
                    with lat_lock:
                        latencies.extend(lats)
            return
        futs = [pool_executor.submit(one_request, base + j)
                for j in range(REQS_PER_STEP)]
        for f in futs:
            f.result()

    def barrier_sync():
        if not args.cpu and torch is not None and torch.cuda.is_available():
            torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()

    for w in range(args.warmup):
        step(w * REQS_PER_STEP)

    barrier_sync()
    timing_on[0] = True
    t_start = time.monotonic()
    for k in range(args.steps):
        if args.dump_outputs and k == args.steps - 1:
            capture_on[0] = True
        step((args.warmup + k) * REQS_PER_STEP)
    timing_on[0] = False
    capture_on[0] = False
    barrier_sync()
    elapsed = time.monotonic() - t_start

    for conn in client_conns:
        try:
            conn.send(("stop",))
        except (BrokenPipeError, OSError):
            pass
    for proc in client_procs:
        proc.join(timeout=5)

    # MAX over ranks
    if dist is not None:
        import torch  # noqa: F811
        te = torch.tensor([elapsed], dtype=torch.float64,
                          device="cuda" if dist.get_backend() == "nccl"
                          else "cpu")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = float(te.item())

    total_requests = args.steps * REQS_PER_STEP * world
    req_per_sec = total_requests / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    loads = sorted(pool.load_durations) or [first_load_s]
    cold_p50 = loads[len(loads) // 2] * 1000.0

    # fast-path stage breakdown (seconds, cumulative over the run)
    stages = {"stage_in": 0, "gpu": 0, "serialize": 0}
    try:
        for e in pool._entries.values():      # noqa: SLF001
            fast = getattr(getattr(e.model, "_gpu", None), "_fast", None)
            if fast is not None:
                si, gp, se = fast.stage_ns()
                stages["stage_in"] += si
                stages["gpu"] += gp
                stages["serialize"] += se
    except Exception:       # noqa: BLE001
        pass
    stages = {k: round(v / 1e9, 3) for k, v in stages.items()}

    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, captured, args.transport,
                      rank, world)

    if rank == 0:
        result = {
            "metric": "predict req/sec (whole node)",
            "value": round(req_per_sec, 2),
            "unit": "req/s",
            "n_gpus": world if not args.cpu else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": (args.dtype if not args.cpu else "f32"),
            "data": "synthetic",
            "config": {
                "model": {"resnet50": "resnet50_v1.5",
                          "mobilenet_v2": "mobilenet_v2",
                          "bert_base": "bert_base",
                          "mixed": "bert_base+resnet50_v1.5"}[args.model],
                "global_batch": args.batch * world,
                "seq_len": args.seq_len if args.model != "resnet50" else args.image_size,
                "parallelism": f"ring-sharded serving x{world}" +
                               (f", replicas={args.replicas}"
                                if eff_mode == "ring" else ""),
                "mode": (f"headline ({eff_mode})" if headline
                         else args.mode),
                "full": bool(args.full),
                "warm_req_per_sec": (round(warm_req_per_sec, 2)
                                     if warm_req_per_sec else None),
                "warm_images_per_sec": (
                    round(warm_req_per_sec * args.batch, 1)
                    if warm_req_per_sec else None),
                "requests_per_step": REQS_PER_STEP,
                "batch_per_request": args.batch,
                "threads": args.threads,
                "images_per_sec": round(req_per_sec * args.batch, 1),
                "n_models": n_models,
                "model_repo": ("hardlinked copies of one SavedModel "
                               "per family (content-dedup applies)"
                               if args.provider == "disk" else
                               "in-process S3-compatible store over "
                               "the same repo (per-object HTTP "
                               "downloads per cold load; content-dedup "
                               "via xxh3 plan keys)"),
                "provider": args.provider,
                "pool_size": pool_cap,
                "cold_load_p50_ms": round(cold_p50, 1),
                "latency_ms": {
                    "p50": round(float(np.percentile(latencies, 50)) * 1e3,
                                 2) if latencies else None,
                    "p95": round(float(np.percentile(latencies, 95)) * 1e3,
                                 2) if latencies else None,
                    "p99": round(float(np.percentile(latencies, 99)) * 1e3,
                                 2) if latencies else None,
                },
                "n_cold_loads": len(loads),
                "transport": {
                    "grpc": "real gRPC (Python grpcio server) over TCP "
                            "loopback",
                    "native": "real gRPC (native nghttp2 front-end) "
                              "over TCP loopback",
                    "native-rest": "real REST (native C++ HTTP/1.1 JSON "
                                   "front-end) over TCP loopback",
                    "inproc": "in-process gRPC message path (protobuf "
                              "decode/encode included)",
                }[args.transport],
                "client_channels": args.channels,
                "fastpath_stage_seconds": stages,
                "hipgraph": _graph_status(pool),
                "dynamic_batching": bool(args.dyn_batch),
            },
        }
        print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""benchlib.common — what every leg of bench.py shares: the roofline peaks, hipGraph capture, the ONE-JSON-line plumbing (straight to stdout, or as records
to a supervisor's pipe), the PMC traffic table, and the test hooks (environment only: PQ_BENCH_TEST_HOOKS, read by tests/ — never a command-line flag)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PEAK_INT8_TOPS = 5033.0     # 256 CU x 4 SIMD x 2048 int8 op/clk x 2.4 GHz (MI355X_MICROARCH.md:28-34,435)
PEAK_HBM_GBS = 8000.0       # spec; 6290 GB/s measured copy (MI355X_MICROARCH.md:36)


def test_hooks():
    """PQ_BENCH_TEST_HOOKS="supervise,native-crash,native-hang,leg-hang=native_overlap2" (tests only): run the tp worker under its supervisor also at one rank; the worker
    kills itself (SIGSEGV) when it reaches the native exchange; the native phase never returns; the named native leg never returns."""
    out = {}
    for item in filter(None, os.environ.get("PQ_BENCH_TEST_HOOKS", "").split(",")):
        k, _, v = item.partition("=")
        out[k.strip()] = v.strip() or True
    return out


def graph_of(fn, n, dev=None):
    """A hipGraph holding n consecutive calls of fn (launched on torch's current stream at replay)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g


def host_cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def med(v):
    return sorted(v)[len(v) // 2]


def traffic_for(shape=None, key=None):
    """HBM bytes per launch / per step from the PMC passes (profiles/traffic.json: rocprofv3 --pmc FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE, separate passes).
    shape = (M, N, K) of a GEMM launch, or key = a workload name ("mlp", "llama8b", "llama70b-shard": per STEP, summed over the step's kernels).  Returns (bytes or None, source)."""
    tj = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        tr = json.load(open(tj))
    except Exception:
        return None, None
    if key is not None:
        w = tr.get("workload_hbm_bytes_per_step", {}).get(key)
        return (w, tr.get("source_by_workload")) if w else (None, None)
    if tuple(shape) == (4096, 4096, 4096):
        return tr.get("gemm_hbm_bytes_per_launch"), tr.get("source")
    v = tr.get("gemm_hbm_bytes_per_launch_by_shape", {}).get("x".join(str(s) for s in shape))
    return (v, tr.get("source_by_shape")) if v else (None, None)


GRAPH_QUEUES = "DEBUG_HIP_FORCE_GRAPH_QUEUES"


def graph_queue_default(environ):
    """The value bench.py gives DEBUG_HIP_FORCE_GRAPH_QUEUES before HIP initialises, or None to leave the runtime alone; a pure function of the environment mapping.
    HIP 7.0 replays a graph with parallel branches (the native_overlap legs of --mode tp fork to the communicator's side stream) on a pool of its own streams, 4 of them by
    default, and while it hands them out it skips every pool stream that shares the launch stream's hardware queue WITHOUT looking for the end of the pool.  On a host that
    caps the hardware queues of a process (GPU_MAX_HW_QUEUES) below 4, several pool streams share that queue, the walk leaves the pool and the first replay dies with SIGSEGV
    inside hipGraphLaunch (met at a cap of 2, in the 4-block leg).  One graph stream needs no pool: "1" under such a cap.  The branches of a forked graph then run in capture
    order on the launch stream — same nodes, same bits, NO overlap (the line says so: config.graph_streams, and the note of each overlap leg).  A value already set wins."""
    cap = str(environ.get("GPU_MAX_HW_QUEUES") or "")
    if environ.get(GRAPH_QUEUES) or not cap.isdigit() or not 0 < int(cap) < 4:
        return None
    return "1"


def apply_graph_queue_default(environ=os.environ):
    """Called at the top of bench.py's main(): after `import torch` (which only loads the HIP library; the runtime reads its switches when it initialises, at the first HIP
    call) and before anything touches the GPU.  Not at import time: a process that merely imports bench keeps its environment.  Returns graph_streams() for the line."""
    v = graph_queue_default(environ)
    if v is not None:
        environ[GRAPH_QUEUES] = v
    return graph_streams(environ)


def graph_streams(environ=os.environ):
    """config.graph_streams of the JSON line: the streams a replayed graph may use (1 = the branches of a forked graph run one after the other), None = the runtime's default"""
    v = str(environ.get(GRAPH_QUEUES) or "")
    return int(v) if v.isdigit() else None


DUMP_BUDGET_BYTES = 60 * 10**6     # --dump-outputs: everything written stays below 64 MB
DUMP_SAMPLE_SEED = 20240607


def sample_rows(n_rows, bytes_per_row, budget_bytes, seed=DUMP_SAMPLE_SEED):
    """The rows of an [n_rows, ...] output that --dump-outputs keeps: all of them when they fit the budget, otherwise a fixed sample — as many rows as fit, drawn
    once from a seeded CPU generator (the same rows on every box and in every run) and sorted."""
    keep = min(n_rows, max(1, budget_bytes // max(1, bytes_per_row)))
    if keep >= n_rows:
        return torch.arange(n_rows)
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n_rows, generator=g)[:keep].sort().values


def dump_outputs(dirpath, arrays, budget_bytes=DUMP_BUDGET_BYTES):
    """--dump-outputs DIR: write what the timed path computed as DIR/<name>.npy, float32 (every value the path produces — bf16 / fp16 / f32 outputs, int8 codes — is
    exact in float32).  `arrays` maps a name to a 1-D or 2-D tensor.  2-D arrays with the same number of rows share ONE row sample (row i of y.npy and of x_codes.npy is the
    same token): the budget left by the 1-D arrays is split evenly over the row counts (what a small group leaves goes to the larger ones), and a group that does not fit is cut down to sample_rows() of
    its rows, the kept row indices beside each array as DIR/<name>_rows.npy.  Returns {file name: shape} for the JSON line."""
    import numpy as np
    os.makedirs(dirpath, exist_ok=True)
    groups = {}
    for name, t in arrays.items():
        if t.dim() == 2:
            groups.setdefault(t.shape[0], []).append(name)
    left = budget_bytes - sum(4 * t.numel() for t in arrays.values() if t.dim() != 2)
    per_row = {n_rows: sum(4 * arrays[n].shape[1] + 4 for n in names) for n_rows, names in groups.items()}       # (+ 4: the row's index in <name>_rows.npy)
    rows_of, rest = {}, left
    for i, n_rows in enumerate(sorted(groups, key=lambda r: r * per_row[r])):      # the smallest first: what a group that fits whole leaves goes to the larger ones
        rows_of[n_rows] = sample_rows(n_rows, per_row[n_rows], rest // (len(groups) - i))
        rest -= rows_of[n_rows].numel() * per_row[n_rows]
    written, total = {}, 0

    def save(name, t):
        nonlocal total
        a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
        np.save(os.path.join(dirpath, name + ".npy"), a)
        written[name + ".npy"] = list(a.shape)
        total += a.nbytes
    for name, t in arrays.items():
        if t.dim() == 2:
            rows, stale = rows_of[t.shape[0]], os.path.join(dirpath, name + "_rows.npy")
            if rows.numel() < t.shape[0]:
                if total + 4 * rows.numel() * (t.shape[1] + 1) > left:
                    raise ValueError(f"--dump-outputs: one row of {name} ({t.shape[1]} values) does not fit what is left of the {budget_bytes}-byte budget")
                save(name + "_rows", rows)
                t = t[rows.to(t.device)]
            elif os.path.exists(stale):
                os.remove(stale)               # (a directory used before, for a larger problem)
        save(name, t)
    return written


def dumped_outputs_entry(dirpath, arrays, what):
    """The line's `dumped_outputs`.  The files are written after every measurement, and a dump that fails then — the directory gone, the disk full — must not lose the line:
    the entry carries the error instead of the files."""
    entry = {"dir": os.path.abspath(dirpath), "dtype": "float32", "what": what}
    try:
        entry["files"] = dump_outputs(dirpath, arrays)
    except Exception as e:
        entry["error"] = f"{type(e).__name__}: {e}"[:300]
        print(f"[bench] --dump-outputs failed: {entry['error']}", file=sys.stderr)
    return entry


_JSON_FD = None


def _claim_stdout():
    """The driver reads ONE JSON line from stdout.  Native libraries write there too (RCCL prints a version banner through C stdio when
    a communicator is created, flushed at exit): from here on file descriptor 1 goes to stderr, and the JSON line alone is written to
    the original stdout (emit_json)."""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


def _pipe_fd():
    v = os.environ.get("PQ_BENCH_PIPE")
    return int(v) if v else None


def emit_json(obj, final=True):
    """The ONE JSON line.  Under a supervisor (tp runs over more than one rank: supervise()) it goes to the supervisor's pipe as a record — provisional lines too,
    so that the best line so far survives a worker that dies — and the supervisor prints the last one; otherwise straight to the original stdout."""
    fd = _pipe_fd()
    if fd is not None:
        os.write(fd, (json.dumps({"final": bool(final), "line": obj}) + "\n").encode())
        return
    if not final:
        return
    data = (json.dumps(obj) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(data.decode()); sys.stdout.flush()
    else:
        os.write(_JSON_FD, data)


def emit_marker(name):
    fd = _pipe_fd()
    if fd is not None:
        os.write(fd, (json.dumps({"marker": name}) + "\n").encode())


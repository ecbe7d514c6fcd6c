"""Time one E-step, one M-step (with relocation) and k-means++ of the device k-means (csrc/kmeans.hip) with HIP events, at the semantic_m shape
N = 2^20 rows, D = 1024, K = 2048 by default; LayerNorm-ed random rows. Also one host Lloyd iteration (sklearn, else numpy) on a subsample, as a baseline.

    python tools/kmeans_bench.py [--n 1048576] [--d 1024] [--k 2048] [--reps 5] [--pp-centres 2048] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiotoken_amd import _cabi  # noqa: E402
from audiotoken_amd import kmeans as KM  # noqa: E402


def timed(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()   # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pp-centres", type=int, default=2048, help="k-means++ is timed over this many centres (the full K by default)")
    ap.add_argument("--host-rows", type=int, default=65536)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a HIP device")
    dev = torch.device("cuda:0")
    n, d, k = a.n, a.d, a.k
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    X = torch.nn.functional.layer_norm(X, (d,))
    x_max = float(X.abs().max())
    lib = _cabi.load()
    h = lib.at_kmeans_create(0, n, d, k)
    assert h, _cabi.last_error()
    res = {"n": n, "d": d, "k": k, "device_bytes": int(lib.at_kmeans_device_bytes(n, d, k)), "gpu": torch.cuda.get_device_name(0)}
    try:
        stream = torch.cuda.current_stream(dev)
        sh = _cabi.current_stream_handle(dev)
        _cabi.check(lib.at_kmeans_set_data(h, X.data_ptr(), x_max, sh), "set_data")
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:k].to(dev)
        C = X[idx].contiguous()
        C_new = torch.empty_like(C)
        labels = torch.empty(n, dtype=torch.int16, device=dev)
        prev = torch.empty_like(labels)
        counts = torch.empty(k, dtype=torch.int32, device=dev)
        stats = torch.zeros(6, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        c_max = float(C.abs().max())

        def e_step():
            _cabi.check(lib.at_kmeans_assign(h, C.data_ptr(), c_max, labels.data_ptr(), status.data_ptr(), sh), "assign")

        def m_step():
            _cabi.check(lib.at_kmeans_update(h, labels.data_ptr(), prev.data_ptr(), C.data_ptr(), C_new.data_ptr(), counts.data_ptr(),
                                             stats.data_ptr(), sh), "update")

        t_e = timed(e_step, a.reps, stream)
        prev.copy_(labels)
        t_m = timed(m_step, a.reps, stream)
        st = stats.cpu().numpy()
        res.update({"e_step_ms": t_e, "m_step_ms": t_m, "e_step_ms_median": float(np.median(t_e)), "m_step_ms_median": float(np.median(t_m)),
                    "m_over_e": float(np.median(t_m) / np.median(t_e)), "status": int(status.cpu()[0]), "n_empty": int(st[3]),
                    "score_gemm_gflop": 2.0 * n * d * ((k + 127) // 128 * 128) / 1e9})
        print(json.dumps({kk: res[kk] for kk in ("e_step_ms_median", "m_step_ms_median", "m_over_e", "n_empty", "status")}), flush=True)
        # the M-step with empty clusters to relocate: two clusters emptied by relabelling their rows to cluster 0
        lab2 = labels.clone()
        lab2[(lab2 == 1) | (lab2 == 2)] = 0

        def m_step_reloc():
            _cabi.check(lib.at_kmeans_update(h, lab2.data_ptr(), prev.data_ptr(), C.data_ptr(), C_new.data_ptr(), counts.data_ptr(),
                                             stats.data_ptr(), sh), "update")

        t_mr = timed(m_step_reloc, a.reps, stream)
        res.update({"m_step_reloc2_ms": t_mr, "m_step_reloc2_ms_median": float(np.median(t_mr)), "reloc_n_empty": int(stats.cpu()[3])})
        print(json.dumps({"m_step_reloc2_ms_median": res["m_step_reloc2_ms_median"], "reloc_n_empty": res["reloc_n_empty"]}), flush=True)
        # k-means++ over the full K (one run; the first launches are part of it)
        trials = KM.n_local_trials(k)
        u = torch.from_numpy(KM.plusplus_uniforms(k, 0)).to(dev)
        picked = torch.empty(k, dtype=torch.int64, device=dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record(stream)
        _cabi.check(lib.at_kmeans_plusplus(h, u.data_ptr(), trials, C_new.data_ptr(), picked.data_ptr(), sh), "plusplus")
        ev1.record(stream)
        ev1.synchronize()
        res.update({"plusplus_ms": ev0.elapsed_time(ev1), "plusplus_trials": trials})
        print(json.dumps({"plusplus_ms": res["plusplus_ms"]}), flush=True)
    finally:
        lib.at_kmeans_destroy(h)
    # host baseline: one Lloyd iteration on a subsample
    m = min(a.host_rows, n)
    Xh = X[:m].cpu().numpy()
    Ch = C.cpu().numpy()
    try:
        from sklearn.cluster import KMeans as SK
        t0 = time.perf_counter()
        SK(n_clusters=k, init=Ch, n_init=1, max_iter=1, algorithm="lloyd", tol=0.0).fit(Xh)
        res["host"] = {"what": "sklearn KMeans(max_iter=1) fit", "rows": m, "s": time.perf_counter() - t0, "threads": os.environ.get("OMP_NUM_THREADS")}
    except ImportError:
        t0 = time.perf_counter()
        dd = (Xh * Xh).sum(1)[:, None] + (Ch * Ch).sum(1)[None, :] - 2.0 * Xh @ Ch.T
        lab = dd.argmin(1)
        np.add.at(np.zeros_like(Ch), lab, Xh)
        res["host"] = {"what": "numpy expanded-form E-step + add.at M-step", "rows": m, "s": time.perf_counter() - t0}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

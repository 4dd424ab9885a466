#!/usr/bin/env python3
"""bench.py -- est-fact on MI355X: one step = one pass of the WHOLE est-fact hot path over one C3
batch (BASELINE.json configs[2]: 200 kb genomic x 100 000 ESTs ~600 bp, 3 % errors) per GPU.

A step runs the product code path (pintron_amd/host/*.c = the est-fact program, as a library):
pairings of all prepared sequences over the device suffix-array index (resident patterns), then
per EST: MEG construction, embedding enumeration, candidate cleaning, filters, intron refinement,
post-refinement -- host C on the worker threads -- with EVERY dynamic program (ALIGN, GAP, ED, KBAND,
LCF, BORDERS, AFFIX) batched across ESTs onto the GPU through the C-ABI (libpintron_gpu.so).  The
step ends with the text of the six output files in host memory (what est-fact writes to
raw-multifasta-out.txt etc.) plus the packed factorization records; for N > 1 the packed records are
gathered to rank 0 over RCCL inside the step.
Not in the step: reading genomic.txt/ests.txt, strand/polyA preparation, index construction (done
once, reported as load_s / index_s), writing the files.

A plain run sets up, warms up, times the steps, writes the last step's outputs (--dump-outputs DIR) and prints
its line.  Everything else is measured and checked with --full only, in the same line: what a user who brings a
NEW batch gets, `fresh_batch` (two distinct batches alternate; reading and preparing the input, building the index,
uploading the patterns and the step are all inside the timed region, every output md5-checked against the
reference's) and `oneshot` (one est-fact process, start to files on disk); `other_workloads`: short legs of
the other single-GPU shares of BASELINE.json (C5 share, C2), md5-checked, each with its own roofline; the md5 of
the timed step's output against the reference's (`timed_output`), the records rank 0 gathered (`gathered`); and
a bounded sample of the same workload run through the reference CPU est-fact (oracle/_ref/est-fact-core, the
cpu_baseline) and through this code, whose two raw-multifasta-out.txt must be byte-identical.

Contract: python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR] ; one JSON line on rank 0.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
N_EST_BATCH = 100_000          # C3
# ESTs per GPU per step of each workload = the share of one GPU of an 8-GPU node in BASELINE.json's configs:
# C2 and C3 whole, one gene of C4 (x genes on the rank), an eighth of C5's two million reads
PER_GPU = {"C2": 1_000, "C3": N_EST_BATCH, "C4": 62_500, "C5": 250_000}
# ESTs of the same workload given to the reference CPU est-fact (about 10-30 s of one core)
CPU_SAMPLE_OF = {"C2": 1_000, "C3": 3_000, "C4": 3_000, "C5": 6_000}
CPU_SAMPLE = CPU_SAMPLE_OF["C3"]


from pintron_amd.estfact import (OUTPUT_FILES, RECORDS, Session, gather_tensor, load_host_lib,  # noqa: E402
                                 parse_factorization_records)
# --dump-outputs: bytes per array (records in float64, texts in float32): 36 + 5 x 4 MiB, under 64 MB in all
DUMP_RECORD_BYTES = {"records_ests": 4 << 20, "records_factorizations": 8 << 20, "records_exons": 24 << 20}
DUMP_TEXT_BYTES = 4 << 20
# processed-megs-info.txt is left out: it holds per-EST timings, as the reference's does
DUMP_TEXTS = [f for f in OUTPUT_FILES if f != "processed-megs-info.txt"]


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as CHILD processes
    (torch.distributed.run, one per GPU) and relay rank 0's JSON line.  Never an exec: under
    rocprofv3 this process already has the GPU initialised.  The parent touches no GPU."""
    import socket
    import torch
    have = torch.cuda.device_count()          # does not initialise the GPU
    if have < args.gpus and os.environ.get("PINTRON_DIST_BACKEND", "nccl") == "nccl":
        raise SystemExit("bench: --gpus %d but %d visible (PINTRON_DIST_BACKEND=gloo lets ranks share GPUs, for tests only)"
                         % (args.gpus, have))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for l in proc.stdout.splitlines():
        if l.startswith("{") and '"metric"' in l:
            line = l
        else:
            print(l, file=sys.stderr)
    if proc.returncode != 0 or line is None:
        raise SystemExit("bench: the %d-rank run failed (exit %d)" % (args.gpus, proc.returncode))
    if json.loads(line)["n_gpus"] != args.gpus:
        raise SystemExit("bench: asked for %d ranks, the run reports %s" % (args.gpus, json.loads(line)["n_gpus"]))
    print(line, flush=True)


def rocprof_symbol(group_name):
    """Kernel symbol (as rocprofv3 prints it) of a kernel group name reported by the library."""
    import re
    modes = {"ED": 0, "ALIGN": 1, "BORDERS": 2, "AFFIX": 3, "KBAND": 4}
    m = re.match(r"lev_wave<(\w+)>$", group_name)                 # every row class in one launch
    if m:
        return "lev_any_kernel<%d, false>" % modes[m.group(1)]    # the common row classes (<= 16 rows per lane)
    m = re.match(r"lev_wave<(\w+),R=1>", group_name)
    if m:
        return "lev_wave_kernel<1, %d, false>" % modes[m.group(1)]
    if group_name == "lev_wave<AFFIX,strips>":
        return "lev_wave_kernel<64, 3, true>"
    return {"dp_batch": "dp_batch_kernel", "wave_jobs": "wave_jobs_kernel", "gap_wave": "gap_any_kernel<false>", "borders_coop": "borders_coop_any_kernel", "affix_coop": "affix_coop_any_kernel",
            "lcf": "lcf_kernel", "align_traceback": "align_traceback_wave_kernel",
            "gap_traceback": "gap_traceback_wave_kernel"}.get(group_name, group_name.split("+")[0] + "_kernel")


def pmc_traffic(group_name, ests_per_launch=None, workload="C3"):
    """HBM bytes per launch of that kernel from the committed PMC passes (tools/pmc_traffic.sh:
    (2 x FETCH_SIZE + WRITE_SIZE) x 1024, separate --pmc runs), or None.  The counter passes run a smaller
    batch whose launches carry a different number of ESTs, so the per-launch figure is scaled to the
    launches of THIS run by ESTs per launch when both are known.  The newest table of the workload wins
    (profiles/rNN_pmc_traffic[_<workload>].json)."""
    import glob
    tag = "" if workload == "C3" else "_" + workload.lower()
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic%s.json" % tag)))
    if not found:
        return None
    path = found[-1]
    sym = rocprof_symbol(group_name)
    table = json.load(open(path))
    run = table.get("_run", {})
    for k, v in table.items():
        if k != "_run" and sym in k:
            per_launch = v["hbm_bytes_per_launch"]
            if ests_per_launch and run.get("ests") and v.get("launches"):
                per_launch *= ests_per_launch / (run["ests"] / v["launches"])
            return per_launch
    return None


def cpu_reference(sample_dir):
    """Reference CPU est-fact (oracle/_ref, compiled from /root/reference) on the sample, one core."""
    exe = os.path.join(ROOT, "oracle", "_ref", "est-fact-core")
    if not os.path.exists(exe):
        return None
    t0 = time.perf_counter()
    subprocess.run([exe], cwd=sample_dir, check=True, stderr=subprocess.DEVNULL)
    return time.perf_counter() - t0


def usable_cores(cap=16):
    """Cores this process may use: affinity mask, cgroup CPU quota (v2 or v1), at most `cap`
    (the host share of one GPU; same rule as the product's default worker count)."""
    n = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, -(-int(q) // int(per)))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and per > 0:
                n = min(n, -(-q // per))
        except (OSError, ValueError):
            pass
    return max(1, min(n, cap))


def cpu_reference_all_cores(n_proc, base_seed, workload="C3", sample=CPU_SAMPLE):
    """The embarrassingly parallel CPU figure: one reference est-fact process per
    usable core, each on its own seeded sample of `sample` ESTs of the workload, all started together."""
    from pintron_amd import synth
    exe = os.path.join(ROOT, "oracle", "_ref", "est-fact-core")
    dirs = []
    for k in range(n_proc):
        d = tempfile.mkdtemp(prefix="pintron_bench_refN_")
        synth.write_files(synth.make(workload, n_est=sample, seed=base_seed + 1000 + k), d)
        dirs.append(d)
    t0 = time.perf_counter()
    procs = [subprocess.Popen([exe], cwd=d, stderr=subprocess.DEVNULL) for d in dirs]
    ok = all(p.wait() == 0 for p in procs)
    wall = time.perf_counter() - t0
    for d in dirs:
        shutil.rmtree(d, ignore_errors=True)
    return wall if ok else None


def kernels_of(stats, steps):
    """per-kernel sums of the sessions' statistics, per step"""
    kernels = {}
    for s in (x for per_step in stats for x in per_step):
        for k in range(s.n_kernels):
            ks = s.kernels[k]
            d = kernels.setdefault(ks.name.decode(), dict(ms=0.0, launches=0, jobs=0, cells=0, algo_bytes=0))
            d["ms"] += ks.ms / steps; d["launches"] += ks.launches / steps
            d["jobs"] += ks.jobs / steps; d["cells"] += ks.cells / steps
            d["algo_bytes"] += ks.algo_bytes / steps
    return kernels


def roofline_of(kernels, n_est, wl):
    """`roofline` object of the dominant kernel + the per-kernel table"""
    name, dom = max(kernels.items(), key=lambda kv: kv[1]["ms"])
    per_launch_ms = dom["ms"] / max(dom["launches"], 1)
    ach = dom["algo_bytes"] / (dom["ms"] * 1e-3) / 1e9 if dom["ms"] and dom["algo_bytes"] else None
    roof = {"bound": "hbm", "kernel": name, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS if ach else None,
            "traffic": pmc_traffic(name, n_est / max(dom["launches"], 1), wl),
            "avg_launch_ms": per_launch_ms, "launches_per_step": dom["launches"],
            "algo_bytes_per_launch": dom["algo_bytes"] / max(dom["launches"], 1)}
    # integer DP: the arithmetic bound is VALU issue, not MFMA.  Chip peak = 256 CU x 4 SIMD x 32
    # lanes/cycle x 2.4 GHz lane-ops/s (MI355X_MICROARCH.md); a unit-cost cell needs >= 6 VALU ops
    if dom["cells"] and dom["ms"]:
        peak_cells = 256 * 4 * 32 * 2.4e9 / 6.0
        ach_cells = dom["cells"] / (dom["ms"] * 1e-3)
        roof["valu"] = {"achieved": ach_cells / 1e9, "peak": peak_cells / 1e9, "unit": "Gcells/s",
                        "frac": ach_cells / peak_cells, "ops_per_cell_assumed": 6}
    table = [{"name": n, "ms_per_step": round(k["ms"], 3), "launches": round(k["launches"], 1),
              "jobs": int(k["jobs"]),
              "algo_GBs": round(k["algo_bytes"] / (k["ms"] * 1e-3) / 1e9, 1) if k["ms"] and k["algo_bytes"] else None,
              # cells (reference loop bounds) per second of this kernel's own stream time
              "Gcells_s": round(k["cells"] / (k["ms"] * 1e-3) / 1e9, 1) if k["ms"] and k["cells"] else None}
             for n, k in sorted(kernels.items(), key=lambda kv: -kv[1]["ms"])]
    return roof, table


def gold_md5(name, n, seed):
    gold_path = os.path.join(ROOT, "tests", "golden", "bench_md5.json")
    if not os.path.exists(gold_path):
        return None
    return json.load(open(gold_path)).get("%s:%d:seed%d" % (name, n, seed))


def sample_rows(a, max_bytes, seed):
    """`a` itself, or a fixed seeded sample of its rows (in their order) when it is larger than max_bytes"""
    import numpy as np
    row = a.itemsize * max(1, int(np.prod(a.shape[1:])))
    if a.nbytes <= max_bytes:
        return a
    idx = np.unique(np.random.default_rng(seed).integers(0, len(a), max_bytes // row))
    return a[idx]


def dump_outputs(directory, records, texts):
    """What the last timed step handed its caller, as DIR/<name>.npy, for comparing two builds output by output:
    the packed factorization records (`records`: per aligned EST [est index, factorizations], per factorization
    [polya, polyad, exons], per exon [est start, est end, genomic start, genomic end]; float64) and the bytes of
    the output texts (`texts`: DUMP_TEXTS -> bytes; float32, their lengths in text_lengths.npy)."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    groups = parse_factorization_records(records)
    arrays = {
        "records_ests": np.array([(e, len(f)) for e, f in groups], dtype=np.float64).reshape(-1, 2),
        "records_factorizations": np.array([(pa, pd, len(ex)) for _, f in groups for pa, pd, ex in f],
                                           dtype=np.float64).reshape(-1, 3),
        "records_exons": np.array([x for _, f in groups for _, _, ex in f for x in ex], dtype=np.float64).reshape(-1, 4)}
    for k, (name, a) in enumerate(arrays.items()):
        np.save(os.path.join(directory, name + ".npy"), sample_rows(a, DUMP_RECORD_BYTES[name], 11 + k))
    lengths = []
    for k, name in enumerate(DUMP_TEXTS):
        b = np.frombuffer(texts[name], dtype=np.uint8)
        lengths.append(len(b))
        np.save(os.path.join(directory, name.replace(".txt", "").replace("-", "_") + ".npy"),
                sample_rows(b, DUMP_TEXT_BYTES // 4, 101 + k).astype(np.float32))
    np.save(os.path.join(directory, "text_lengths.npy"), np.array(lengths, dtype=np.float64))


def other_workload_leg(L, synth, wl, steps=5, warmup=2):
    """A short leg of another single-GPU share of BASELINE.json (its own session, closed afterwards): the same
    measurement as the headline -- steps timed between synchronisations, output md5 against the reference's,
    roofline of its dominant kernel -- in the default command's line, so that it is timed where the headline is."""
    import torch
    n, seed = PER_GPU[wl], synth.CONFIGS[wl]["seed"]
    work = tempfile.mkdtemp(prefix="pintron_bench_%s_" % wl.lower())
    try:
        synth.write_files(synth.make(wl, n_est=n, seed=seed), work)
        sess = Session(L, work)
        try:
            for _ in range(warmup):
                sess.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = [[sess.step()] for _ in range(steps)]
            torch.cuda.synchronize()
            step_s = (time.perf_counter() - t0) / steps
            st = stats[-1][0]
            md5 = hashlib.md5(sess.records()).hexdigest()
            gold = gold_md5(wl, sess.n_ests(), seed)
            if gold and md5 != gold["raw-multifasta-out.txt"]:
                raise SystemExit("bench: the timed step's raw-multifasta-out of %s differs from the reference's" % wl)
            leg = {"workload": "%s: %d ESTs per GPU (seed %d)" % (wl, sess.n_ests(), seed), "steps": steps, "warmup": warmup,
                   "ms_per_step": step_s * 1e3, "value": int(st.aligned) / step_s, "unit": "aligned ESTs/s",
                   "input_ests_per_s": sess.n_ests() / step_s,
                   "timed_output": {"md5": md5, "reference_md5": gold["raw-multifasta-out.txt"] if gold else None,
                                    "identical_to_reference": bool(gold) and md5 == gold["raw-multifasta-out.txt"]},
                   "phases_s": {"prefetch_pairings": st.prefetch_s, "workers_wall": st.workers_s,
                                "host_cpu_per_thread": st.host_s / st.threads, "dp_batches_per_thread": st.dp_s / st.threads},
                   "suspensions_per_est": st.suspensions_per_unit,
                   "kernel_busy_union_ms": sum(x[0].dp_busy_union_ms for x in stats) / steps}
            kernels = kernels_of(stats, steps)
            if kernels:
                leg["roofline"], leg["kernels"] = roofline_of(kernels, sess.n_ests(), wl)
                leg["kernels"] = leg["kernels"][:4]
            return leg
        finally:
            sess.close()
    finally:
        shutil.rmtree(work, ignore_errors=True)


def fresh_batch_leg(L, synth, wl, n, seeds, rounds=2):
    """What a user who brings a new batch gets, inside one process: the batches of `seeds` alternate, and for each
    of them reading + preparing the input, building the index, uploading the patterns, the step itself and the
    release of the session are inside the timed region (the input files are written before).  Every output is
    compared with the reference's checksum for that batch."""
    import torch
    dirs = []
    for sd in seeds:
        d = tempfile.mkdtemp(prefix="pintron_bench_fresh_")
        synth.write_files(synth.make(wl, n_est=n, seed=sd), d)
        dirs.append(d)
    checks, times, aligned = [], [], 0
    try:
        torch.cuda.synchronize()
        for r in range(rounds):
            for sd, d in zip(seeds, dirs):
                t0 = time.perf_counter()
                sess = Session(L, d)
                st = sess.step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                md5 = hashlib.md5(sess.records()).hexdigest()          # (copying the text out and checking it is not timed)
                t2 = time.perf_counter()
                sess.close()
                t_step = (t1 - t0) + (time.perf_counter() - t2)
                times.append(t_step)
                aligned = int(st.aligned)
                gold = gold_md5(wl, n, sd)
                ok = bool(gold) and md5 == gold["raw-multifasta-out.txt"]
                if gold and not ok:
                    raise SystemExit("bench: fresh batch %s:%d:seed%d differs from the reference's output" % (wl, n, sd))
                checks.append({"batch": "%s:%d:seed%d" % (wl, n, sd), "seconds": t_step, "identical_to_reference": ok if gold else None})
    finally:
        for d in dirs:
            shutil.rmtree(d, ignore_errors=True)
    warm = times[len(seeds):] or times                 # the first visit of each batch also pages the code in
    ms = 1e3 * sum(warm) / len(warm)
    return {"ms_per_step": ms, "value": aligned / (ms * 1e-3), "unit": "aligned ESTs/s", "input_ests_per_s": n / (ms * 1e-3),
            "what": "two distinct batches alternate; per batch: read + prepare ests.txt / genomic.txt, build the index, upload, "
                    "one step, close -- all timed; the first round (first visit of each batch) is not averaged",
            "batches": checks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ests", type=int, default=None, help="ESTs per GPU per step (default: the workload's per-GPU share, PER_GPU)")
    ap.add_argument("--genes", type=int, default=None, help="C4 only: number of genes (default 8 = BASELINE.json configs[3]; 1 = one GPU's share)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the checks against the reference's output, the one-process and fresh-batch "
                         "legs, the other workloads' legs and the CPU baseline (off: set up, warm up, time, print)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float64 / float32, < 64 MB in all)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the cpu_baseline / parity leg")
    ap.add_argument("--no-oneshot", action="store_true", help="--full without the one-process start-to-files measurement")
    ap.add_argument("--no-extra", action="store_true", help="--full without the fresh-batch leg and the other workloads' legs (N = 1, default workload only)")
    ap.add_argument("--workload", choices=("C2", "C3", "C4", "C5"), default="C3",
                    help="C3 (default, the metric's configuration): one 200 kb gene x --ests per GPU; "
                         "C4: 8 genes x 200 kb, --ests ESTs each (62 500 = BASELINE.json configs[3]), gene g on rank g mod N; "
                         "C2: 50 kb x 1 000 ESTs; C5: 1 Mb x 250 000 reads of 150 bp per GPU (an eighth of configs[4])")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.ests is None:
        args.ests = PER_GPU[args.workload]

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    # one rank per GPU over RCCL.  PINTRON_DIST_BACKEND=gloo (as in pintron_amd.multi) keeps the
    # exchange on the host and lets the ranks share GPUs: the way to exercise the N > 1 flow of this
    # file on a box with fewer GPUs than ranks
    backend = os.environ.get("PINTRON_DIST_BACKEND", "nccl")
    dev_index = local if world > 1 else 0
    if backend != "nccl":
        dev_index = local % max(torch.cuda.device_count(), 1)
    xdev = "cuda" if backend == "nccl" else "cpu"
    os.environ["PINTRON_GPU_DEVICE"] = str(dev_index)
    os.environ.setdefault("PINTRON_KERNEL_TIMING", "1")
    dist = None
    # (without a GPU only the CPU tests get past the next lines -- gloo + the check build of the host library,
    # PINTRON_ESTFACT_LIB; the product library refuses to open a session when there is no gfx950 device)
    have_gpu = backend == "nccl" or torch.cuda.is_available()
    if have_gpu:
        torch.cuda.set_device(dev_index)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from pintron_amd import synth
    L = load_host_lib()
    wl = args.workload
    if wl != "C4":
        # every rank gets its own batch (weak scaling); rank r uses seed <config seed> + r so batches differ
        genes = [(wl, synth.CONFIGS[wl]["seed"] + rank, args.ests)]
    else:
        # C4: eight independent est-fact problems; gene g runs on rank g mod N (strong scaling)
        n_genes = args.genes or synth.CONFIGS["C4"]["genes"]
        # (a rank without a gene -- fewer genes than ranks -- takes part in every collective with nothing to send)
        genes = [("C4", synth.CONFIGS["C4"]["seed"] + g, args.ests) for g in range(n_genes) if g % world == rank]
    works, sessions = [], []
    for name, seed, n in genes:
        work = tempfile.mkdtemp(prefix="pintron_bench_r%d_" % rank)
        synth.write_files(synth.make(name, n_est=n, seed=seed), work)
        works.append(work)
        sessions.append(Session(L, work))
    n_est = sum(s.n_ests() for s in sessions)

    gathered = {}

    def step():
        sts = [sess.step() for sess in sessions]
        if world > 1:
            # the only exchange of the sharded path: the factorization records of the rank's ESTs
            # (packed: 16 B per exon + 4 B per factorization, everything downstream stages parse out
            # of raw-multifasta-out.txt) -> rank 0 over RCCL.  ONE gather per step whatever the number
            # of genes on the rank (ranks with different gene counts, or none, issue the same collectives)
            recs = [sess.output_tensor(RECORDS) for sess in sessions]
            mine = torch.empty(0, dtype=torch.uint8) if not recs else (recs[0] if len(recs) == 1 else torch.cat(recs))
            parts = gather_tensor(mine, dist, rank, world, xdev)
            if parts is not None:
                gathered["parts"] = parts
        return sts

    def fence():
        if world > 1:
            dist.barrier()
        if have_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    stats = [step() for _ in range(args.steps)]
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=xdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    total_est = n_est
    n_aligned = total_aligned = int(sum(x.aligned for x in stats[-1])) if stats[-1] else 0
    if world > 1:
        tn = torch.tensor([n_est, n_aligned], dtype=torch.int64, device=xdev)
        dist.all_reduce(tn)
        total_est, total_aligned = int(tn[0].item()), int(tn[1].item())
    if rank == 0 and args.dump_outputs:
        # the sharded path hands rank 0 the records of every rank; the texts are those of rank 0's own genes
        records = b"".join(bytes(p.cpu().numpy().tobytes()) for p in gathered["parts"]) if world > 1 else \
            b"".join(sess.output(RECORDS) for sess in sessions)
        dump_outputs(args.dump_outputs, records,
                     {f: b"".join(sess.output(OUTPUT_FILES.index(f)) for sess in sessions) for f in DUMP_TEXTS})
    if rank == 0:
        st = stats[-1][-1]
        kernels = kernels_of(stats, args.steps)
        step_s = dt / args.steps
        out = {
            "metric": "ESTs aligned/sec (whole node) + DP Mcells/s; bit-exact factorizations vs ref",
            "metric_version": 2,          # since round 3 `value` counts ALIGNED ESTs (the metric's wording); input ESTs/s is beside it
            # the metric says "ESTs ALIGNED per second": the ESTs that got at least one factorization (what
            # processed-ests.txt lists); the input rate is beside it
            "value": total_aligned / step_s, "unit": "aligned ESTs/s", "input_ests_per_s": total_est / step_s,
            "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": step_s * 1e3, "higher_is_better": True,
            "scaling": "weak" if wl != "C4" else "strong", "vs_baseline": None, "dtype": "u8/int32", "data": "synthetic",
            "config": {"workload": {"C3": "C3: 200 kb genomic x %d ESTs ~600 bp, 3%% errors, per GPU" % n_est,
                                    "C2": "C2: 50 kb genomic x %d ESTs ~500 bp, 1%% errors, per GPU" % n_est,
                                    "C5": "C5: 1 Mb genomic x %d reads of 150 bp, 1%% errors, per GPU (BASELINE.json configs[4] = 8 such shares)" % n_est,
                                    "C4": "C4: %d genes x 200 kb, %d ESTs ~600 bp each, gene g on rank g mod %d (%d ESTs in all)"
                                          % (args.genes or synth.CONFIGS["C4"]["genes"], genes[0][2], world, total_est)}[wl],
                       "stages": "whole est-fact hot path per step: GPU pairings over the device index + host MEG/"
                                 "embeddings/filters/refinement (%d threads, fibres) with all DPs batched on the GPU"
                                 % st.threads,
                       "ests_per_gpu": n_est, "aligned_per_gpu": n_aligned,
                       "dp_jobs_per_step": int(sum(x.dp_jobs for x in stats[-1])),
                       "dp_batches_per_step": int(sum(x.dp_batches for x in stats[-1])),
                       "parallelism": "est-shard x%d" % world},
            "dp_mcells_per_s": sum(k["cells"] for k in kernels.values()) * world / step_s / 1e6,
            "phases_s": {"load_once": st.load_s, "index_once": st.index_s, "prefetch_pairings": st.prefetch_s,
                         "workers_wall": st.workers_s, "host_cpu_per_thread": st.host_s / st.threads,
                         "dp_batches_per_thread": st.dp_s / st.threads},
            # times an EST gave up its thread to wait for answers from the device, per input EST
            "suspensions_per_est": st.suspensions_per_unit,
            # the kernels' ms_per_step below are sums over launches that overlap in time (several service streams);
            # this is the time the device spent in DP kernels with all launches on one time line: <= ms_per_step
            "kernel_busy_union_ms": sum(x.dp_busy_union_ms for per_step in stats for x in per_step) / args.steps,
        }
        # the text the LAST TIMED step left on rank 0 against the reference's checksum for the very same
        # batch (tools/make_bench_md5.py ran the reference object code on it in the build container)
        if args.full:
            out["timed_output_md5"] = hashlib.md5(b"".join(sess.records() for sess in sessions)).hexdigest()
        gold_path = os.path.join(ROOT, "tests", "golden", "bench_md5.json")
        if args.full and os.path.exists(gold_path):
            # every gene of this rank whose batch has a committed checksum (C4: gene 0 = one GPU's share)
            table = json.load(open(gold_path))
            checked = []
            for (name, seed, n), sess in zip(genes, sessions):
                gold = table.get("%s:%d:seed%d" % (name, sess.n_ests(), seed))
                if not gold:
                    continue
                md5 = hashlib.md5(sess.records()).hexdigest()
                checked.append({"batch": "%s:%d:seed%d" % (name, sess.n_ests(), seed), "md5": md5,
                                "reference_md5": gold["raw-multifasta-out.txt"], "identical_to_reference": md5 == gold["raw-multifasta-out.txt"]})
                if md5 != gold["raw-multifasta-out.txt"]:
                    raise SystemExit("bench: the timed step's raw-multifasta-out of %s differs from the reference's (md5 %s vs %s)"
                                     % (checked[-1]["batch"], md5, gold["raw-multifasta-out.txt"]))
            if checked:
                out["timed_output"] = dict(checked[0], ests=n_est, batches_checked=len(checked))
        if args.full and world == 1 and wl != "C4" and not args.no_oneshot:
            # the way the pipeline driver uses est-fact (dist-scripts/pintron.py:878-884): one process per
            # gene, process start -> the six files on disk.  Outside the timed steps; the resident
            # sessions above keep their HBM.
            exe = os.path.join(ROOT, "pintron_amd", "bin", "est-fact")
            t_one = time.perf_counter()
            rc_one = subprocess.run([exe], cwd=works[0], stderr=subprocess.DEVNULL).returncode
            t_one = time.perf_counter() - t_one
            if rc_one == 0:
                raw = open(os.path.join(works[0], "raw-multifasta-out.txt"), "rb").read()
                out["oneshot"] = {"seconds": t_one, "ESTs_per_s": n_est / t_one,
                                  "what": "est-fact process start -> six files on disk, same %d-EST batch" % n_est,
                                  "md5_equals_timed_step": hashlib.md5(raw).hexdigest() == out["timed_output_md5"]}
        if args.full and world > 1 and "parts" in gathered:
            # what rank 0 holds after the last step's gather: the record groups of every rank (one per aligned EST)
            from pintron_amd.estfact import parse_factorization_records
            sizes = [int(p.numel()) for p in gathered["parts"]]
            groups = sum(len(parse_factorization_records(bytes(p.cpu().numpy().tobytes()))) for p in gathered["parts"])
            out["gathered"] = {"bytes_per_rank": sizes, "est_groups": groups, "equals_aligned": groups == total_aligned}
            if groups != total_aligned:
                raise SystemExit("bench: rank 0 received %d record groups for %d aligned ESTs" % (groups, total_aligned))
        if kernels:
            out["roofline"], out["kernels"] = roofline_of(kernels, n_est, wl)
        if args.full and world == 1 and wl == "C3" and args.ests == PER_GPU["C3"] and not args.no_extra:
            # the resident sessions above are done: their HBM and threads go before the other legs start
            for sess in sessions:
                sess.close()
            sessions = []
            out["fresh_batch"] = fresh_batch_leg(L, synth, "C3", args.ests, [synth.CONFIGS["C3"]["seed"], 1003])
            out["other_workloads"] = [other_workload_leg(L, synth, w2) for w2 in ("C5", "C2")]
        if args.full and world == 1 and not args.no_cpu:
            # bounded sample of the same workload: reference CPU est-fact vs this code, byte for byte
            cpu_n = min(CPU_SAMPLE_OF[wl], n_est)
            sample = synth.make(wl, n_est=cpu_n, seed=genes[0][1])
            sdir_ref = tempfile.mkdtemp(prefix="pintron_bench_ref_")
            sdir_gpu = tempfile.mkdtemp(prefix="pintron_bench_gpu_")
            synth.write_files(sample, sdir_ref)
            synth.write_files(sample, sdir_gpu)
            cpu_s = cpu_reference(sdir_ref)
            if cpu_s is not None:
                s2 = Session(L, sdir_gpu)
                s2.step()
                got = s2.records()
                s2.close()
                ref = open(os.path.join(sdir_ref, "raw-multifasta-out.txt"), "rb").read()
                if got != ref:
                    raise SystemExit("bench: GPU est-fact output differs from the reference CPU est-fact on the sample")
                # counted like `value`: ESTs the reference aligned (its processed-ests.txt) per second
                ref_aligned = open(os.path.join(sdir_ref, "processed-ests.txt"), "rb").read().count(b">")
                frac = ref_aligned / max(cpu_n, 1)
                out["cpu_baseline"] = {"value": ref_aligned / cpu_s, "unit": "aligned ESTs/s", "input_ests_per_s": cpu_n / cpu_s,
                                       "cores": 1, "kind": "reference",
                                       "sample": "first-seed %s sample of %d ESTs (%d aligned) through oracle/_ref/est-fact-core "
                                                 "(%.1f s, its suffix-tree build included); output byte-identical to this code's"
                                                 % (wl, cpu_n, ref_aligned, cpu_s)}
                n_proc = usable_cores()
                wall_all = cpu_reference_all_cores(n_proc, synth.CONFIGS[wl]["seed"], wl, cpu_n) if n_proc > 1 else None
                if wall_all:
                    out["cpu_baseline"]["all_cores"] = {
                        "value": frac * n_proc * cpu_n / wall_all, "unit": "aligned ESTs/s (aligned share of the first sample assumed)",
                        "input_ests_per_s": n_proc * cpu_n / wall_all, "cores": n_proc,
                        "sample": "%d reference processes side by side, %d ESTs each (%.1f s)" % (n_proc, cpu_n, wall_all)}
                out["parity"] = {"sample_ests": cpu_n, "raw_multifasta_md5": hashlib.md5(ref).hexdigest(), "identical": True}
            shutil.rmtree(sdir_ref, ignore_errors=True)
            shutil.rmtree(sdir_gpu, ignore_errors=True)
        print(json.dumps(out), flush=True)
    for sess in sessions:
        sess.close()
    for work in works:
        shutil.rmtree(work, ignore_errors=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

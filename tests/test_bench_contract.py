"""bench.py prints ONE JSON line with the fields the driver reads (metric / value / unit / ..., roofline, cpu_baseline),
the roofline describes the kernel that dominates a fresh kernel trace, and the other configurations produce a line too."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(extra), capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    d = _bench("--full", "--steps", "40", "--warmup", "10", "--secondary-steps", "20")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "timed_region_s", "step_ms_p50", "step_ms_p95",
                "value_device_images", "value_sync_ctor_host_images", "value_with_pose_opt", "fps_formula", "prewarm_steps", "parity"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 10
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 0.01 * d["value"]
    assert abs(d["timed_region_s"] - 40 * d["ms_per_step"] * 1e-3) < 0.02 * d["timed_region_s"]
    assert 0 < d["step_ms_p50"] <= d["step_ms_p95"]
    assert 0 < d["value_sync_ctor_host_images"] and 0 < d["value_device_images"] and 0 < d["value_with_pose_opt"] < d["value"] * 1.2
    assert d["prewarm_steps"] >= 200 and d["fps_formula"] > 0
    cfgd = d["config"]
    # `value` is the host-image accounting: the images enter through pinned staging + a PCIe copy inside the step
    assert cfgd["host_images_in_step"] is True and "pinned staging" in cfgd["image_ingest"]
    assert cfgd["local_map_keyframes"] == 20 and 2000 <= cfgd["local_map_points_avg"] <= 12000 and cfgd["sequence_frames"] >= 190
    assert d["data"] == "synthetic" and "workload" in cfgd and "model" not in cfgd and cfgd["name"] == "C2"
    assert cfgd["device_copy_GBps_measured"] > 500 and cfgd["host_cpu"]["nproc"] >= 1 and cfgd["host_cpu"]["model"]
    assert cfgd["whole_step_hbm"]["achieved_GBps"] > 0
    # what the (shared) host did to the region: involuntary context switches of the process's threads, neighbours on the agent's cores
    assert "nonvoluntary_ctxt_switches_in_region" in cfgd["host_noise"]
    rf = d["roofline"]
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "bracketed_launches"):
        assert key in rf, key
    assert rf["bound"] in ("hbm", "mfma") and rf["peak"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-6
    assert rf["bracketed_launches"] >= 2 and 0.002 < rf["avg_launch_ms"] < 1.0      # (one solve in four carries the event pair)
    cb = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample", "build", "host_cpu"):
        assert key in cb, key
    assert cb["kind"] in ("reference", "port") and cb["value"] > 0 and cb["cores"] >= 1
    # the in-job parity gate: 20 frames of the timed sequence through libagentloop.so against the oracle
    pr = d["parity"]
    assert pr["ok"] is True and pr["frames"] == 20 and pr["extract_bit_exact"] and pr["stereo_bit_exact"] and pr["match_frame_equal"]
    assert pr["match_map_equal"] and pr["lba_iters_equal"] and pr["lba_max_abs"] <= 1e-4 and "libagentloop" in pr["loop"]
    # ... and the closed loop: 200 frames through the reference-signature glue, product and oracle each on their own outputs
    cl = pr["closed_loop"]
    assert cl["ok"] is True and cl["frames"] == 200 and cl["keyframes"] == 40 and cl["first_divergent_frame"] == -1 and cl["first_divergent_frame_no_caches"] == -1
    assert cl["shadow_calls"] >= 1800 and cl["shadow_mismatches"] == 0 and cl["shadow_max_lba_abs_diff"] <= 1e-4
    rl = pr["rig_closed_loop"]
    assert rl["ok"] is True and rl["frames"] == 120 and rl["max_pose_diff"] <= 1e-3 and rl["max_match_entries_differing_in_a_frame"] <= 8
    assert rl["shadow"]["ok"] is True and rl["shadow"]["mismatches"] == 0 and rl["shadow"]["calls"] > 700
    # ... and both optimisers on a two-fisheye rig (parity-only leg: no BASELINE configuration has a second camera)
    rg = pr["camera_rig"]
    assert rg["ok"] is True and rg["lba_right_camera_edges"] > 500 and rg["lba_iterations_equal"] and rg["lba_max_pose_diff"] <= 1e-4
    assert rg["pose_opt_max_pose_diff"] <= 1e-5
    # ... and Tracking's matchers on a two-camera frame of that rig
    assert rg["frustum_flags_and_levels_equal"] and rg["search_map_points_features_differing"] == 0 and rg["search_last_frame_features_differing"] == 0
    assert rg["search_map_points_matches"][0] == rg["search_map_points_matches"][1] > 300
    assert rg["fisheye_partner_arrays_equal"] and rg["fisheye_stereo_matches"][0] == rg["fisheye_stereo_matches"][1] > 150


@pytest.mark.gpu
def test_roofline_kernel_is_the_top_row_of_a_fresh_kernel_trace():
    """The kernel the roofline describes must be the one with the largest total time in a rocprofv3 kernel trace of the same
    command (serial accounting, so that every kernel of the step is in one trace)."""
    if shutil.which("rocprofv3") is None:
        pytest.skip("rocprofv3 not on PATH")
    out = tempfile.mkdtemp(prefix="orbg_trace_")
    env = dict(os.environ, TMPDIR="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
           sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "60", "--warmup", "10", "--no-cpu-baseline", "--no-secondary",
           "--lba-mode", "inline", "--no-pipeline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd="/tmp", env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    assert stats, os.listdir(out)
    rows = list(csv.DictReader(open(stats[0])))
    # PoseOptimization runs only in the informational tail of bench.py (not in a step): leave it out of the ranking
    rows = [x for x in rows if "pose_opt_kernel" not in x["Name"]]
    # copies are not kernels of the library
    rows = [x for x in rows if "__amd_rocclr" not in x["Name"]]
    rows.sort(key=lambda x: -float(x["TotalDurationNs"]))
    # bench.py picks the subject from its own event brackets; two kernels within 15 % of each other in total time (at the
    # moment octree_kernel and the LDL^T) may swap places between two runs, so the subject has to be the top row or tied with it
    name = d["roofline"]["kernel"].split("::")[-1]
    mine = [x for x in rows if name in x["Name"]]
    assert mine, (name, [x["Name"][:60] for x in rows[:4]])
    assert float(mine[0]["TotalDurationNs"]) >= 0.85 * float(rows[0]["TotalDurationNs"]), (name, [(x["Name"][:50], x["TotalDurationNs"]) for x in rows[:4]])
    # and the live event-bracket duration agrees with the trace's average for that kernel
    avg_us = float(mine[0]["AverageNs"]) / 1e3
    assert abs(1e3 * d["roofline"]["avg_launch_ms"] - avg_us) < 0.25 * avg_us, (d["roofline"]["avg_launch_ms"], avg_us)
    per = d["config"]["device_ms_per_step_by_kernel"]
    assert list(per)[0].split("::")[-1] == name and len(per) >= 5
    shutil.rmtree(out, ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C4", "mono", "mono_dist"])
def test_other_configurations_produce_a_line(name):
    d = _bench("--full", "--config", name, "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--secondary-steps", "10")
    assert d["config"]["name"] == name and d["value"] > 0 and d["config"]["lba_ms_per_call"] > 0
    assert d["roofline"]["bracketed_launches"] >= 1
    assert d["parity"]["ok"] is True and d["parity"]["frames"] == 20          # the in-job gate runs for every configuration
    if name == "C4":
        assert d["roofline"]["unknowns"] == 300 and "k_ldlt_xcd" in d["roofline"]["kernel"]       # (ORBG_LDLT_XCD=0: k_ldlt_big48)
    else:
        # a monocular agent is a first-class agent: fused constructor, pipelined, the C++ loop
        assert d["config"]["host_images_in_step"] is True and "libagentloop" in d["config"]["tracking_loop"]
        assert d["config"]["frame_ctor_ahead"] >= 1 and d["parity"]["stereo_bit_exact"] is None


@pytest.mark.gpu
def test_server_tick_goes_through_rccl_on_one_rank():
    d = _bench("--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-secondary", "--server-tick")
    st = d["config"]["server_tick"]
    assert st["2_kf_blocks_us"] > 0 and st["8_kf_blocks_us"] > st["2_kf_blocks_us"] and "nccl" in st["note"]
    assert 0 < st["exchange_only_8_blocks_us"] < st["8_kf_blocks_us"] and "ONE RCCL all-gather" in st["note"]


@pytest.mark.gpu
def test_cxx_tracking_loop_does_the_work_of_the_python_loop():
    """bench.py times libagentloop.so (csrc/agent_loop.cpp).  On a short sequence the C++ loop and the step-by-step Python loop over
    the same handles must do the same work: identical keypoint and match totals per region for the pipelined host-image,
    pipelined device-image and synchronous constructors, and the same number of local BAs with the same LM iterations."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from multi_orbslam3_amd import _capi as capi, agent, api, synth, views
    cfg = dict(bench.CONFIGS["C2"])
    scene = synth.Scene(640, 480, seed=synth.SEED_IMAGES)
    n_frames = 12
    ex, imgs, host_imgs, frames, kf_chunks, _fv0, _bounds = bench.build_workload(scene, cfg, n_frames, api, views, synth, 0)
    p = scene.frame_view_params()
    fv, _k = views.frame_view(np.zeros(1, capi.KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), None, None, p["bounds"], p["cam"], 8, 1.2)
    exs = [ex] + [api.ORBextractor(cfg["n_features"], 1.2, 8, 20, 7, 640, 480, n_cams=2) for _ in range(3)]     # a ring of four (handle, frame) pairs
    Fs = [api.Frame(cfg["frame_cap"]) for _ in range(4)]
    LM = api.LocalMap(cfg["map_cap"])
    opt = api.Optimizer()
    prob = synth.make_lba_problem(n_free=6, n_fixed=3, n_points=300, seed=5)
    lp, keep = views.lba_problem(prob["poses"], prob["pose_fixed"], prob["points"], prob["edges"], prob["cam"])
    lba_out = views.LbaOutput(lp.n_poses, lp.n_points, lp.n_edges)
    seq = list(range(n_frames)) + list(range(n_frames - 2, 0, -1))
    K = bench.FRAMES_PER_KF
    period = int(np.lcm(len(seq), K))
    sim = bench.LocalMaps(kf_chunks, cfg["local_kfs"], views)
    sim.prefill(seq, 0)
    kf_views = []
    for i in range(2 * period):
        if seq[i % len(seq)] % K == 0:
            sim.visit(seq[i % len(seq)])
        if i % K == 0 and i >= period:
            kf_views.append(sim.view())
    bf, bb = float(scene.cam["bf"]), float(scene.cam["b"])
    frames_in = [dict(host=host_imgs[k], dev=(imgs[k][0].data_ptr(), imgs[k][1].data_ptr()),
                      guess=np.ascontiguousarray(frames[k]["guess"], np.float32).reshape(16), last_view=frames[k]["last_view"][0]) for k in range(n_frames)]
    po = synth.make_pose_opt_problem(n=100, seed=3)
    po1, kp = views.pose_opt_problem(po["Xw"], po["u"], po["v"], po["ur"], po["inv_sigma2"], po["cam"], po["Tcw"])
    loop = agent.AgentLoop(exs, Fs, LM, opt, fv, 640, 480, 640, bf, bb, frames_in, seq, kf_views, lp, lba_out, [po1, po1], K, 2 * cfg["frame_cap"], 7.0, False)
    m_frame, m_map = api.ORBmatcher(0.9, True), api.ORBmatcher(0.8, True)
    n_steps = 23

    def python_region(pipelined, host):
        kp = mf = mm = 0
        amp = np.full(2 * cfg["frame_cap"], -1, np.int32); aob = np.zeros(2 * cfg["frame_cap"], np.int32)
        LM.upload(kf_views[0])
        for i in range(n_steps):
            k, k_last = seq[i % len(seq)], seq[(i - 1) % len(seq)]
            c = i % 4 if pipelined else 0
            if host:
                nl, nr = exs[c].frame_stereo(Fs[c], fv, host_imgs[k][0], host_imgs[k][1], bf, bb, download=False)
            else:
                nl, nr = exs[c].frame_stereo_dev(Fs[c], fv, imgs[k][0].data_ptr(), imgs[k][1].data_ptr(), 640, 480, 640, bf, bb)
            a, b = amp[:nl], aob[:nl]
            a.fill(-1); b.fill(0)
            a, b, n1 = m_frame.SearchByProjectionFrame(Fs[c], frames[k]["guess"], frames[k_last]["last_view"][0], 7.0, False, a, b, inplace=True)
            a, b, n2 = m_map.SearchLocalPoints(Fs[c], LM, frames[k]["guess"], 1.0, False, 0.0, a, b, None, inplace=True)
            if i % K == 0:
                LM.upload(kf_views[(i // K) % len(kf_views)])
            kp += nl + nr; mf += n1; mm += n2
        return kp, mf, mm

    # (frames handed over ahead of the tracked one: 1 = rounds 1-3, 2 = bench.py's default, 3 = the whole ring in flight; submit
    # order before / after the collection of the current frame; a region split over two calls keeps its frames in flight across them)
    for pipelined, host, ahead, first, split in ((True, True, 1, True, False), (True, True, 2, True, True), (True, True, 3, False, False),
                                                 (True, False, 2, False, True), (True, False, 1, True, False), (False, True, 1, True, False)):
        LM.upload(kf_views[0])
        loop.configure(pipelined, host, ingest_async=host, submit_first=first, lba_async=True, pose_opt=False, ahead=ahead)
        if split:
            st = loop.run(0, 9, last_is_final=False, timed=True)
            assert sum(loop.c.in_flight) == (ahead if pipelined else 0)
            st = loop.run(9, n_steps - 9, last_is_final=True, timed=True, stats=st)
        else:
            st = loop.run(0, n_steps, last_is_final=True, timed=True)
        assert sum(loop.c.in_flight) == 0                 # a final region hands nothing over beyond its last step
        loop.drain(st, True)
        torch.cuda.synchronize()
        want = python_region(pipelined, host)
        assert (st.kp, st.m_frame, st.m_map) == want, (pipelined, host, ahead, (st.kp, st.m_frame, st.m_map), want)
        assert st.lba_calls == (n_steps + K - 1) // K and st.lba_iters == st.lba_calls * sum(lba_out.iters)
        assert st.m_frame > 100 * n_steps // 2 and st.kp > 1500 * n_steps


@pytest.mark.gpu
def test_two_ranks_produce_one_aggregate_line():
    """The N > 1 path of bench.py as the driver launches it (torch.distributed.run, one process per rank), here with both ranks on
    the box's one GPU (ORBG_BENCH_SHARE_GPU=1: the rate is meaningless, the code path is the real one): gloo control plane, barrier
    on both sides of the timed region, MAX over ranks, rank 0 prints ONE line whose value is the aggregate over the agents and
    which carries every agent's CPU baseline."""
    port = 29500 + (os.getpid() % 400)
    env = dict(os.environ, ORBG_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "40", "--warmup", "10",
                        "--no-secondary", "--no-dropin"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 40 and d["scaling"] == "weak"
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]          # whole-job aggregate = 2 agents x steps / max time
    assert len(d["cpu_baseline"]["per_agent"]["values"]) == 2


def test_gpus_flag_is_never_silently_ignored():
    """`--gpus N` must produce a line with n_gpus == N or fail: without a launcher bench.py starts the N ranks itself (refused, rc 2,
    when the node has fewer GPUs -- this container has none), and under a launcher whose WORLD_SIZE differs from --gpus it refuses too.
    Both decisions are taken before anything touches a GPU, so they run here."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ORBG_BENCH_SHARE_GPU")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=env)
    if r.returncode == 0:                                  # (a box with >= 2 GPUs: the line must say so)
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert d["n_gpus"] == 2
    else:
        assert r.returncode == 2 and "--gpus 2 but this node has" in r.stderr and not r.stdout.strip()
    env2 = dict(env, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "5"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=env2)
    assert r.returncode == 2 and "refusing" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_self_launched_ranks_and_the_in_job_parity_gate():
    """`python bench.py --gpus 2` with no launcher (how the driver starts N = 1): two rank processes on the box's one GPU
    (ORBG_BENCH_SHARE_GPU=1), ONE line with n_gpus == 2, and the in-job parity gate green for both agents."""
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}, ORBG_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "20", "--warmup", "5", "--no-secondary",
                        "--no-dropin", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 20
    pr = d["parity"]
    assert pr["ok"] is True and pr["agents_ok"] == [True, True] and pr["frames"] == 20
    for key in ("extract_bit_exact", "stereo_bit_exact", "match_frame_equal", "match_map_equal", "lba_iters_equal", "lba_outliers_equal"):
        assert pr[key] is True, key
    assert pr["lba_max_abs"] <= 1e-4 and pr["lba_trace_max_rel"] <= 1e-9 and pr["keypoints_checked"] > 30000


@pytest.mark.gpu
def test_eight_ranks_dry_run_of_the_c5_job_on_a_shared_gpu():
    """`python bench.py --gpus 8 --config C5` exactly as it would be typed on an 8-GPU node, here with all eight ranks on the box's one GPU
    (ORBG_BENCH_SHARE_GPU=1; the server tick's exchange then goes through gloo): the launcher counts the GPUs without loading the HIP
    runtime, eight rank processes come up, ONE line with n_gpus == 8 comes back, the mixed mono / stereo agent kinds of configs[4] are
    in place, every agent's in-job parity gate is green, and the line says where every rank ran (rank -> GPU -> NUMA node -> CPUs).
    The rate it prints says nothing -- eight agents share one GPU and this box's CPU quota; the code path is the 8-GPU one."""
    common = ["--full", "--steps", "20", "--warmup", "5", "--no-secondary", "--no-dropin", "--no-cpu-baseline", "--repeats", "1", "--prewarm-steps", "20"]
    d = _run_bench(["--config", "C5", "--gpus", "8"] + common, share=True, timeout=1500)
    assert d["n_gpus"] == 8 and d["config"]["name"] == "C5" and len(d["config"]["agents"]) == 8 and set(d["config"]["agents"]) == {"stereo", "mono"}
    pr = d["parity"]
    assert pr["ok"] is True and pr["agents_ok"] == [True] * 8 and len(set(pr["agent_digests"])) >= 2 and pr["server_tick"]["ok"] is True
    pl = d["config"]["placement_per_rank"]
    assert [p["rank"] for p in pl] == list(range(8)) and all(p["device"] == 0 and p["cpus"] for p in pl)
    assert d["config"]["server_tick_in_job"]["ticks"] >= 1


def _last_json_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    assert stdout.strip().splitlines()[-1].startswith("{"), "the JSON line must be the last line of the output"
    return json.loads(lines[0])


def _run_bench(args, share=False, timeout=1200):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ORBG_BENCH_SHARE_GPU")}
    if share:
        env["ORBG_BENCH_SHARE_GPU"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return _last_json_line(r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("config,agent1", [("C3", "C2"), ("C5", "mono")])
def test_c3_and_c5_two_agents_with_the_server_tick_in_the_same_job(config, agent1):
    """BASELINE configs[2] / configs[4] as runnable jobs, here with two ranks on the box's one GPU (ORBG_BENCH_SHARE_GPU=1: the exchange
    then goes through gloo over host copies -- RCCL refuses two ranks on one device; the 1-rank run below goes through RCCL):
    per-rank agent kinds, the server tick's collective inside the timed region, the server's outputs equal to the oracle's, and
    SURVEY Appendix F "Multi-GPU": every agent's outputs equal the 1-rank run of the same agent (no cross-talk)."""
    common = ["--full", "--steps", "40", "--warmup", "5", "--no-secondary", "--no-dropin", "--no-cpu-baseline", "--repeats", "1"]
    d = _run_bench(["--config", config, "--gpus", "2"] + common, share=True)
    assert d["n_gpus"] == 2 and d["config"]["name"] == config
    assert d["config"]["agents"] == (["stereo", "stereo"] if config == "C3" else ["stereo", "mono"])
    st = d["config"]["server_tick_in_job"]
    assert st["ticks"] >= 4 and st["blocks"] == 2 * 2 * st["ticks"] and st["database_keyframes"] == 40 and "gloo" in st["exchange"]
    pr = d["parity"]
    assert pr["ok"] is True and pr["agents_ok"] == [True, True] and pr["server_tick"]["ok"] is True and pr["server_tick"]["blocks"] == 4
    for key in ("wire_equal", "bow_equal", "candidates_equal", "bow_matches_equal", "projection_matches_equal"):
        assert pr["server_tick"][key] is True, key
    # each agent alone, same seed: identical outputs (the digest covers keypoints, descriptors, stereo data, both match arrays, the local BA)
    d0 = _run_bench(["--config", "C2", "--first-agent", "0"] + common)
    d1 = _run_bench(["--config", agent1, "--first-agent", "1"] + common)
    assert pr["agent_digests"][0] == d0["parity"]["agent_digests"][0] and pr["agent_digests"][1] == d1["parity"]["agent_digests"][0]
    assert pr["agent_digests"][0] != pr["agent_digests"][1]


@pytest.mark.gpu
def test_c3_server_tick_goes_through_rccl_in_the_timed_region():
    """One rank: the tick's all-gather is an RCCL collective on device memory (a single-rank group), inside the timed region, next to the
    agent; the server's results of the last tick equal the oracle's."""
    d = _run_bench(["--full", "--config", "C3", "--steps", "60", "--warmup", "5", "--no-secondary", "--no-dropin", "--no-cpu-baseline", "--repeats", "1"])
    st = d["config"]["server_tick_in_job"]
    assert "RCCL" in st["exchange"] and st["ticks"] >= 6 and st["exchange_us_per_tick"] > 0 and st["server_us_per_tick"] > 0
    assert d["parity"]["ok"] is True and d["parity"]["server_tick"]["ok"] is True and d["value"] > 0


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_the_last_steps_outputs():
    """`bench.py --gpus 1 --steps N --warmup W` without --full: the headline fields, exactly N timed steps, none of the --full legs;
    --dump-outputs writes the last timed step's outputs as float32 / float64 .npy files, the same in two runs with the same arguments."""
    import numpy as np
    dirs = [tempfile.mkdtemp(prefix="orbg_dump_") for _ in range(2)]
    lines = [_bench("--gpus", "1", "--steps", "30", "--warmup", "5", "--dump-outputs", dd) for dd in dirs]
    for d in lines:
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in d, key
        assert d["steps"] == 30 and d["warmup"] == 5 and d["unit"] == "frames/s" and d["higher_is_better"] is True
        assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 0.01 * d["value"]
        for key in ("roofline", "cpu_baseline", "value_device_images", "value_dropin"):
            assert key not in d, key
        assert d["parity"] is None and d["value_regions"] == 1
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    for want in ("kps_x.npy", "desc.npy", "uright.npy", "depth.npy", "map_point_match.npy", "lba_poses.npy", "lba_points.npy"):
        assert want in names, want
    total = 0
    for nm in names:
        a, b = (np.load(os.path.join(dd, nm)) for dd in dirs)
        assert a.dtype in (np.float32, np.float64), (nm, a.dtype)
        assert np.array_equal(a, b), nm
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(dirs[0], "kps_x.npy")).size > 500 and (np.load(os.path.join(dirs[0], "map_point_match.npy")) >= 0).sum() > 100
    # ... and they are the LAST timed step's: the C++ loop's main region starts at a multiple of the sequence period, so its last step
    # tracks frame seq[(steps - 1) % len(seq)]; the CPU oracle on that frame's images gives the features and stereo data bit for bit
    from multi_orbslam3_amd import synth
    from oracle import binding as ob
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS["C2"]
    n_seq = lines[0]["config"]["sequence_frames"]
    n_frames = n_seq // 2 + 1
    seq = list(range(n_frames)) + list(range(n_frames - 2, 0, -1))
    assert len(seq) == n_seq
    sc = synth.Scene(cfg["W"], cfg["H"], seed=synth.SEED_IMAGES)           # agent 0
    L, R, _ = sc.stereo_pair(seq[(30 - 1) % n_seq])
    exL, exR = (ob.Extractor(n_features=cfg["n_features"], max_width=cfg["W"], max_height=cfg["H"]) for _ in range(2))
    _, okl, odl, _ = exL.extract(L)
    _, okr, odr, _ = exR.extract(R)
    our, odp = ob.stereo_match(exL, exR, okl, odl, okr, odr, float(sc.cam["bf"]), float(sc.cam["b"]))
    got = {nm[:-4]: np.load(os.path.join(dirs[0], nm)) for nm in names}
    assert got["kps_x"].size == len(okl)
    for f in okl.dtype.names:
        assert np.array_equal(got["kps_" + f], okl[f].astype(got["kps_" + f].dtype)), f
    assert np.array_equal(got["desc"], odl.astype(np.float32))
    assert np.array_equal(got["uright"], our[:len(okl)]) and np.array_equal(got["depth"], odp[:len(okl)])
    for dd in dirs:
        shutil.rmtree(dd, ignore_errors=True)

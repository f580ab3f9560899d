#!/usr/bin/env python3
"""bench.py -- complex-IQ Msamples/s through the full chain (BASELINE.json metric) on N MI355X.

One "step" = one pmr_chain_process_block_device() call: one block of synthetic cf32 IQ, already resident in
HBM, through dc-block -> resample -> NCO -> M-channel polyphase channelizer -> NBFM discriminator for all M
channels -> CTCSS high-pass -> gain -> de-emphasis -> int16 PCM (left in HBM).  Consecutive steps are NOT
synchronised: they pipeline on the chain's two HIP streams, as a streaming receiver would run them.  The path shards
by independent IQ stream: rank r owns stream r on GPU r, no data-path collective (torch.distributed is used only for
the start/stop barrier and the max-over-ranks of the elapsed time).

Headline workload (N = 1 and N > 1): cfg5 = BASELINE.json configs[4], the largest single-GPU configuration (the metric
is quoted on no configuration; BASELINE.md calls cfg5 the HBM-roofline config).

A plain run (`bench.py --gpus N --steps K --warmup W`) does only what the headline needs: set-up, W warm-up steps, ONE timed
region of exactly K steps between barrier + synchronize (`value`, `ms_per_step`), the outputs of the last timed step if
`--dump-outputs DIR` is given, and the line.

`--full` adds everything else, as before: the timed region is REPEATED `--regions` times (default 25; `value` /
`ms_per_step` are the median region, `timed_regions` lists first / min / median / max), kernel events and the roofline, the
one-open-channel leg, the PCIe-inclusive host-buffer rates, the CPU baseline, and "also" sub-records -- at N = 1 cfg2
(configs[1]) and cfg3 (configs[2]), each with its own roofline and parity check; at N > 1 cfg3 on every GPU = cfg4
(configs[3]: N independent 61.44 MS/s streams, one per GPU).  Outside the timed regions every workload is checked against
the CPU oracle (`parity_checked`): un-synchronised pipelined calls on the bench block, int16 PCM within +-1 LSB; a failed
check fails the run.

Prints ONE JSON line on rank 0 (see the driver contract in the task statement).
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (fs_in, M, default log2 block, BASELINE.json configs index)
    "cfg2": (2.4e6, 16, 26, 1),      # 16-ch PMR446 chain @ 2.4 MS/s on one MI355X
    "cfg3": (61.44e6, 256, 26, 2),   # 256-ch channelizer + NBFM @ 61.44 MS/s (cfg4 = this, one stream per GPU)
    "cfg5": (1.0e9, 1024, 26, 4),    # 1024-ch channelizer + demod @ 1 GS/s -- HBM-roofline config
}
HEADLINE = "cfg5"
EVENT_EVERY = 8        # timed region: at least every 8th front-end launch carries start/stop events (fewer when that still gives ~24 samples)
HBM_PEAK_GBPS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
KERNEL_SYMBOLS = ("profile slots name the kernels as a rocprofv3 trace does: k_fe_fast<MODE,N3,TAIL> = the specialised front end (MODE 1 = level 1 "
                  "of the two-level form; k_frontend<NT,SPT,MODE> for cascades it does not cover); audio FIR <hp> = k_fir_fft<4, DUAL> on "
                  "large blocks, k_fir_mfma4<...> otherwise")
DUMP_BYTES = 64 << 20  # --dump-outputs: at most this much in all (shared by the ranks)


def dump_outputs(d, arrays, budget):
    """--dump-outputs: each array as float32 d/<name>.npy.  One larger than `budget` bytes is replaced by a fixed sample of its
    elements (seed 0, sorted flat indices): two builds run with the same arguments still compare element for element."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float32)
        if a.nbytes > budget:
            idx = np.unique(np.random.default_rng(0).integers(0, a.size, budget // a.itemsize))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(d, name + ".npy"), a)


def _oracle_loop(fs, M, block_host, seconds_target, only_channel=-1):
    import oracle
    n_probe = min(len(block_host), 1 << 20)
    n_avail = max(1, len(block_host) // n_probe)
    ch = oracle.OracleChain(fs_in=fs, num_channels=M, max_block=n_probe, only_channel=only_channel)
    ch.process_block(block_host[:n_probe], want=("pcm",))               # warm-up (page-in, caches)
    n_blocks = 0
    t0 = time.perf_counter()
    while True:                                                         # same stream continued; sample re-used cyclically
        b = n_blocks % n_avail
        ch.process_block(block_host[b * n_probe:(b + 1) * n_probe], want=("pcm",))
        n_blocks += 1
        dt = time.perf_counter() - t0
        if dt >= seconds_target:
            break
    ch.close()
    return n_blocks, n_probe, dt


_WORKER = """
import sys, time, numpy as np
sys.path.insert(0, %r)
import bench
fs, M, n, secs = float(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4])
from sdr_pmr446_amd import synth
x = synth.synth_iq(n, fs, M, stream_id=int(sys.argv[5]), channels=list(range(0, M, max(1, M // 16))))
nb, npr, dt = bench._oracle_loop(fs, M, x, secs, only_channel=int(sys.argv[6]))
print(nb * npr, dt)
"""


def _native_oracle():
    """Build the oracle with -march=native ON THIS MACHINE (bit-identical to the portable build, see
    oracle/Makefile) for the cpu_baseline workers.  Returns (path or None, flags string)."""
    import subprocess
    try:
        subprocess.check_call(["make", "-B", "-C", os.path.join(ROOT, "oracle"), "-s", "native"], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL, timeout=120)
        p = os.path.join(ROOT, "oracle", "liboracle_pmr_native.so")
        if os.path.exists(p):
            return p, "gcc -O3 -march=native -ffp-contract=off"
    except Exception:
        pass
    return None, "gcc -O3 -ffp-contract=off (portable build; -march=native build failed on this box)"


def cpu_baseline(fs, M, seconds_target=8.0, multi=True):
    """Time the CPU oracle (kind 'port': the reference itself needs liquid-dsp and cannot be built here) on a
    bounded sample of the same workload (1 Msample blocks of the same synthetic channel plan, one process per stream):
    (i) single thread like the reference's DSP thread (src/sdr_pmr446.c:788) -- the headline `value`; (ii) N independent
    streams on N cores, the CPU analogue of one stream per GPU; (iii) the reference's own semantics, one
    squelch-selected channel demodulated (:876-877)."""
    import subprocess
    lib, flags = _native_oracle()
    env = dict(os.environ)
    if lib:
        env["PMR_ORACLE_LIB"] = lib
    n_probe = 1 << 20
    host_cores = os.cpu_count() or 1

    def workers(count, secs, only):
        procs = [subprocess.Popen([sys.executable, "-c", _WORKER % ROOT, str(fs), str(M), str(n_probe), str(secs), str(i),
                                   str(only)], stdout=subprocess.PIPE, cwd=ROOT, env=env) for i in range(count)]
        outs = [p.communicate(timeout=300)[0].split() for p in procs]
        return [(float(o[0]), float(o[1])) for o in outs]

    (tot, dt), = workers(1, seconds_target, -1)
    out = {"value": tot / dt / 1e6, "unit": "Msamples/s", "cores": 1, "kind": "port", "host_cores": host_cores,
           "build": flags,
           "sample": "%d blocks x %d samples of the same synthetic channel plan, all %d channels demodulated, %.1f s" %
                     (int(tot) // n_probe, n_probe, M, dt)}
    (tot1, dt1), = workers(1, seconds_target / 2, 0)
    out["one_channel"] = {"value": tot1 / dt1 / 1e6, "cores": 1,
                          "sample": "reference semantics: only the selected channel demodulated, %.1f s" % dt1}
    try:
        ncores = len(os.sched_getaffinity(0)) if multi else 1           # every core this process may use
        if ncores > 1:
            rates = [t / d for t, d in workers(ncores, seconds_target / 2, -1)]
            out["multi"] = {"value": sum(rates) / 1e6, "cores": ncores,
                            "sample": "%d independent streams, one single-threaded oracle per core (host has %d cores)"
                                      % (ncores, host_cores)}
    except Exception as e:                                              # the single-thread figure stands on its own
        out["multi"] = {"value": None, "error": str(e)[:120]}
    return out


def load_measured_traffic(workload, block):
    """HBM bytes per launch of the roofline kernel from the rocprofv3 PMC passes committed under profiles/
    (FETCH_SIZE doubled per MI355X_MICROARCH.md, + WRITE_SIZE), if they were taken for this workload/block -- and whether they were
    taken with THESE kernels: the entry carries the sha256 of the kernel sources it was measured on (tools/collect_profiles.sh);
    a different tree keeps the number and marks it stale.  Returns (bytes or None, stale flag or None, round tag or None)."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        with open(path) as f:
            t = json.load(f)
        e = t.get("%s/k_frontend/%d" % (workload, block))
        if not e:
            return None, None, None
        from sdr_pmr446_amd import build as _b
        return e["hbm_bytes_per_launch"], e.get("kernel_sources_sha256") != _b.kernel_sources_sha256(), e.get("round")
    except Exception:
        return None, None, None


def parity_check(ch, fs, M, iq, block, pcm_bufs, S, nblk, rot=1, sabotage=False):
    """Outside the timed region: `nblk` consecutive process_block_device calls on the bench stream (the rotation's blocks in
    order), NOT synchronised in between (the timed code path), PCM of every call vs the CPU oracle fed the same stream."""
    import numpy as np
    import oracle
    from sdr_pmr446_amd import synth
    from sdr_pmr446_amd import parity_rule
    x_host = iq.download(np.complex64, min(rot, nblk) * block)
    ref, ref_chan, ref_fm, err = [], [], [], []

    def run_oracle():
        try:
            chunk = 1 << 22
            o = oracle.OracleChain(fs_in=fs, num_channels=M, max_block=chunk)
            for b in range(nblk):
                base = (b % rot) * block
                for p in range(0, block, chunk):
                    first = b == 0 and p == 0
                    r = o.process_block(x_host[base + p:base + p + chunk], want=("pcm", "chan", "fm") if first else ("pcm", "chan"))
                    ref.append(r["pcm"]); ref_chan.append(r["chan"])
                    if first:
                        ref_fm.append(r["fm"])
            o.close()
        except Exception as e:                                          # reported below, never swallowed
            err.append(repr(e))

    th = threading.Thread(target=run_oracle)                            # ctypes releases the GIL: the oracle runs beside the GPU
    t0 = time.perf_counter()
    th.start()
    ch.reset()
    ns = []
    for b in range(nblk):
        ns.append(ch.process_block_device(iq.ptr + (b % rot) * block * 8, block, d_pcm=pcm_bufs[b].ptr, stride=S))
    ch.synchronize()
    got = np.concatenate([pcm_bufs[b].download(np.int16, M * S).reshape(M, S)[:, :ns[b]] for b in range(nblk)],
                         axis=1).astype(np.int32)
    # the chain's discriminator output of the stream's first frames, through the debug tap of a second, small handle (same device;
    # the capture selects the in-place form of the dc carry, bit-identical: tests/test_gpu_carry.py): what parity_rule needs to tell an
    # ill-conditioned arg() from an error
    from sdr_pmr446_amd import chain as pmr
    nfirst = min(block, 1 << 22)
    gd = pmr.PmrChain(fs_in=fs, num_channels=M, max_block=nfirst, device=ch.cfg.device)
    fm_got = gd.process_block(x_host[:nfirst], want=("fm",))["fm"]
    gd.close()
    th.join()
    if err:
        return {"ok": False, "error": err[0]}
    if sabotage:                                       # --test-fail-rank: this rank's PCM is falsified so that its check MUST fail
        got = got + 3
    ref = np.concatenate(ref, axis=1).astype(np.int32)
    ref_chan = np.concatenate(ref_chan, axis=1)
    act = synth.signal_channels(M, fs)            # not empty, not inside the chain's own dc-block notch (ill-conditioned)
    n_empty = sum(synth.channel_kind(k) == "empty" for k in range(M))
    if got.shape != ref.shape:
        return {"ok": False, "error": "frame count: chain %r, oracle %r" % (got.shape, ref.shape)}
    # +-1 LSB, except where the audio filter's response to an ILL-CONDITIONED discriminator sample reaches (the check starts at a reset):
    # there the PCM must equal the oracle's plus what the measured discriminator difference at those samples explains
    # (sdr_pmr446_amd/parity_rule.py) -- a rule on measured quantities, not a blanket time window (VERDICT r05 weak #1a)
    hp, b0, b1, a1 = parity_rule.fixtures(ROOT)
    h = parity_rule.audio_response(hp, ch.cfg.audio_gain, b0, b1, a1)
    F = min(fm_got.shape[1], ref_fm[0].shape[1])
    v = parity_rule.check(got[act], ref[act], ref_chan[act], fm_got[act][:, :F], ref_fm[0][act][:, :F], h)
    if "error" in v:
        return {"ok": False, "error": v["error"]}
    ok = v["ok"]
    return {"ok": bool(ok), "max_abs_pcm_diff_lsb": v["max_abs_pcm_diff_lsb"], "tolerance_lsb": 1, "blocks": nblk,
            "ill_conditioned": v["ill_conditioned"],
            "dc_notch_channels_excluded": M - len(act) - n_empty, "empty_channels_excluded": n_empty,
            "block_samples": block, "frames_checked": int(got.shape[1]), "channels_checked": len(act),
            "channels_excluded": "%d empty (noise only) + %d inside the dc-block notch (|H_dc| < 0.5): discriminator ill-conditioned"
                                 % (n_empty, M - len(act) - n_empty),
            "within_1_lsb_frac_all_channels": float((np.abs(got - ref) <= 1).mean()) if ok else None,
            "mode": "consecutive process_block_device calls, no synchronisation in between, block pipelining on",
            "input": "blocks 0..%d of the timed rotation, in order" % (min(rot, nblk) - 1) if rot > 1 else "the bench block, repeated",
            "oracle": "oracle.OracleChain (CPU restatement) on the same %d samples" % (nblk * block),
            "seconds": round(time.perf_counter() - t0, 1)}


def measure(name, args, rank, local_rank, world, dist, dev, headline, dump=None):
    """One workload: synth the block in HBM, warm up, time `regions` x K un-synchronised steps, write the last step's outputs
    to `dump` if given; with --full also the per-kernel breakdown, the other legs and the parity check.  Returns the record
    (rank 0) or None."""
    import torch
    from sdr_pmr446_amd import chain as pmr
    from sdr_pmr446_amd import multigpu

    fs, M, lb, cfg_idx = WORKLOADS[name]
    lb = args.log2_block if args.log2_block is not None else lb
    block = 1 << lb
    ch = pmr.PmrChain(fs_in=fs, num_channels=M, max_block=block, device=local_rank)
    if args.ctcss:
        ch._check(ch._L.pmr_chain_ctcss_enable(ch.h, 1))
    S = ch.max_frames
    # Resident in HBM before timing, generated there by the library's own kernel (include/pmr_mem.h: every buffer of this
    # program lives in the library's HIP runtime; torch is here for torch.distributed only).  period_log2: all frequencies
    # snapped to the block's grid, so the block repeated every step is one phase-continuous stream.
    # The timed steps ROTATE through `rot` distinct blocks (one phase-continuous stream of rot x block samples whose every frequency is
    # snapped to the grid of the whole rotation, so block rot-1 runs into block 0 without a phase step; the noise is a counter-based
    # stream of its own): a streaming receiver never sees the same block twice, and a block re-read every step next to a 256 MiB
    # Infinity Cache would leave open how much of the "HBM" stream the cache served.
    rot = max(1, args.rotate)
    rot_log2 = rot.bit_length() - 1
    if rot != 1 << rot_log2:
        raise SystemExit("--rotate must be a power of two")
    iq = pmr.synth_iq_device(rot * block, fs, M, stream_id=multigpu.stream_id_for_rank(rank), period_log2=lb + rot_log2,
                             device=local_rank)
    nchk = max(1, args.parity_blocks) if args.full else 1
    pcm_bufs = [pmr.DeviceBuffer(M * S * 2, local_rank) for _ in range(nchk)]                # PCM stays in HBM
    pcm = pcm_bufs[0]
    pmr.device_synchronize()

    def device_sync():
        torch.cuda.synchronize()
        pmr.device_synchronize()

    pos = [0, rot, 0]                                 # [next block of the rotation, blocks in the rotation (1 = same block every step),
                                                      #  frames of the last step]

    def step():
        b = pos[0] % pos[1]
        pos[0] += 1
        pos[2] = ch.process_block_device(iq.ptr + b * block * 8, block, d_pcm=pcm.ptr, stride=S)
        return pos[2]

    for _ in range(args.warmup):
        step()
    ch.synchronize()
    ch.profile_reset()
    # HIP events in the timed region only on the roofline kernel (the front end), as start/stop events its launch carries
    # (the kernel's own begin..end) on every EVENT_EVERY-th launch: event RECORDS around every front-end launch are two
    # marker packets on the critical stream and cost 11 % of the step (cfg5: 0.146 vs 0.132 ms, tools/steps_ab.sh);
    # the full per-kernel breakdown is taken right after, outside the timed region
    n_regions = max(1, args.regions if headline or world == 1 else 1)
    # a launch that carries events costs a marker packet on the critical stream (~1 % of the step at one in eight): thin them out
    # to ~24 samples over the whole measurement, never denser than one in EVENT_EVERY nor sparser than one in 32
    event_every = max(EVENT_EVERY, min(32, (n_regions * args.steps) // 24))
    import math
    while math.gcd(event_every, args.steps) != 1:      # ... and coprime with the region length: the sampled launch must walk through
        event_every += 1                               # every position of a region (a region's first front end has the GPU to itself)
    ch.profile_enable(1 + event_every if args.full and not args.no_kernel_events else 0)

    def run():
        n = 0
        for _ in range(args.steps):
            n += step()
        ch.synchronize()
        return n

    sync_dev = None                                   # (the Dist object knows where its MAX-reduce tensor lives)
    dts, frames = [], 0
    for _ in range(n_regions):
        dt, frames = multigpu.timed_region(run, dist, device_sync, sync_dev)
        dts.append(dt)
    ch.profile_enable(0)
    prof_roof = ch.profile()
    if dump:                                          # what a caller of the timed path receives from its last step: int16 PCM [M][frames]
        import numpy as np
        dump_outputs(dump, {"pcm" if rank == 0 else "pcm_rank%d" % rank:
                            pcm.download(np.int16, M * S).reshape(M, S)[:, :pos[2]]}, DUMP_BYTES // world)
    # the same measurement on ONE block re-read every step (rounds 1-3's input), for the record: 5 regions
    dts_same = []
    if args.full and rot > 1:
        pos[1] = 1
        dts_same = [multigpu.timed_region(run, dist, device_sync, sync_dev)[0] for _ in range(5)]
        pos[1] = rot
    breakdown_steps = 0
    if args.full and not args.no_kernel_events:
        # separate pass, outside the timed region: every kernel, blocks NOT pipelined (uncontended kernel times)
        ch.set_overlap(False)
        ch.profile_reset()
        ch.profile_enable(1)
        breakdown_steps = min(args.steps, 5)
        for _ in range(breakdown_steps):
            step()
        ch.synchronize()
        ch.profile_enable(0)
        ch.set_overlap(True)
    prof = ch.profile()
    # the reference's own semantics (src/sdr_pmr446.c:876-877): one squelch-selected channel demodulated to audio
    from sdr_pmr446_amd import synth as _synth
    dts1 = []
    if args.full and not args.no_one_open:
        one = _synth.signal_channels(M, fs)[0]
        ch.set_channel_mask([one])
        for _ in range(args.warmup):
            step()
        ch.synchronize()
        dts1 = [multigpu.timed_region(run, dist, device_sync, sync_dev)[0] for _ in range(5)]
        ch.set_channel_mask(None)

    # Every rank checks ITS stream on ITS device against the oracle (un-synchronised pipelined calls on the bench blocks): N = 1 the
    # whole rotation, N > 1 two 2^26-sample blocks per rank (~3-4 s of one host core each, the ranks run in parallel on their
    # NUMA-local cores); the verdicts are AND-reduced over the gloo group.  Without this an 8-GPU run would return eight throughput
    # numbers and no evidence that device ordinals 1-7 compute the right thing (per-device hipSetDevice, table uploads, streams).
    par = None
    if args.full and args.parity_blocks > 0:
        par = parity_check(ch, fs, M, iq, block, pcm_bufs, S, nchk if world == 1 else min(2, nchk), rot,
                           sabotage=args.test_fail_rank == rank)
        par["device"] = local_rank
        par_all = multigpu.reduce_parity(dist, rank, world, par)
        par.update(par_all)
    rec = None
    if rank == 0:
        r = M * 12500.0 / fs
        b_alg = 8.0 + 2.0 * r                                        # bytes per input sample
        dt_med = statistics.median(dts)
        value = multigpu.aggregate_throughput(world, args.steps, block, dt_med) / 1e6
        roof = None
        if prof_roof:
            kname, (ms, n) = max(prof_roof.items(), key=lambda kv: kv[1][0])
            avg_s = ms / n * 1e-3
            launches_per_step = n / (args.steps * len(dts))
            achieved = b_alg * block / avg_s / 1e9
            traffic, stale, tround = load_measured_traffic(name, block)
            roof = {"bound": "hbm", "kernel": kname, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_stale": stale,
                    "traffic_source": None if traffic is None else "profiles/traffic.json (%s PMC passes: not measured in this run; "
                                      "traffic_stale = the kernel sources differ from the ones the passes ran on)" % tround,
                    "avg_kernel_ms": ms / n, "launches_timed": n, "launches_per_step": launches_per_step,
                    "events": "start/stop events carried by every %d-th launch of the kernel inside the timed regions" % event_every,
                    "algorithmic_bytes_per_sample": b_alg, "algorithmic_bytes_per_launch": b_alg * block,
                    "kernel_symbols": KERNEL_SYMBOLS,
                    "kernels_ms_per_step_isolated": {k: v[0] / max(1, breakdown_steps) for k, v in sorted(prof.items())}}
            iso = prof.get(kname)
            if iso and iso[1]:
                iso_s = iso[0] / iso[1] * 1e-3
                roof["isolated"] = {"avg_kernel_ms": iso[0] / iso[1], "achieved": b_alg * block / iso_s / 1e9,
                                    "frac": b_alg * block / iso_s / 1e9 / HBM_PEAK_GBPS,
                                    "note": "same kernel with block pipelining off (no other kernel sharing the GPU)"}
        ms_all = [d / args.steps * 1e3 for d in dts]
        rec = {
            "value": value, "unit": "Msamples/s", "ms_per_step": dt_med / args.steps * 1e3,
            "timed_regions": {"n": len(dts), "steps_each": args.steps, "ms_per_step_first": ms_all[0],
                              "ms_per_step_min": min(ms_all), "ms_per_step_median": statistics.median(ms_all),
                              "ms_per_step_max": max(ms_all), "value_is": "median region",
                              "input": ("%d distinct device-resident blocks (%.2f GB, one phase-continuous stream, period 2^%d samples) "
                                        "rotated through the steps" % (rot, rot * block * 8 / 1e9, lb + rot_log2)) if rot > 1
                                       else "one device-resident block re-read every step",
                              "same_block_every_step": ({"value": multigpu.aggregate_throughput(world, args.steps, block,
                                                                                                 statistics.median(dts_same)) / 1e6,
                                                         "ms_per_step": statistics.median(dts_same) / args.steps * 1e3, "regions": len(dts_same),
                                                         "note": "block 0 of the rotation re-read every step (the input of rounds 1-3)"}
                                                        if dts_same else None)},
            "config": {"workload": ("cfg4 (BASELINE.json configs[3]): %d independent %d-ch streams @ %.4g MS/s, one per GPU (cfg3 on "
                                    "every GPU)" % (world, M, fs / 1e6)) if (name == "cfg3" and world > 1) else
                                   ("%s (BASELINE.json configs[%d]): %d-ch PMR446 chain @ %.4g MS/s, one independent IQ "
                                    "stream per GPU" % (name, cfg_idx, M, fs / 1e6)),
                       "block_samples": block, "frames_per_step": frames // max(1, args.steps),
                       "channels_demodulated": M,
                       "hbm_frac_of_peak_whole_chain": value * 1e6 * b_alg / 1e9 / world / HBM_PEAK_GBPS},
            "roofline": roof,
            "one_open_channel": None if not dts1 else {"value": multigpu.aggregate_throughput(world, args.steps, block, statistics.median(dts1)) / 1e6,
                                 "ms_per_step": statistics.median(dts1) / args.steps * 1e3, "open_channels": 1, "regions": len(dts1),
                                 "note": "reference semantics (src/sdr_pmr446.c:876-877): channelizer + discriminator for all %d "
                                         "channels, audio FIR / PCM for the one open channel (pmr_chain_set_channel_mask)" % M},
        }
        if not args.full:                                            # a plain run measured neither
            del rec["roofline"], rec["one_open_channel"]
        if par is not None:
            rec["parity_checked"] = par
        if args.full and headline and not args.no_host_io and world == 1:
            rec["host_io"] = host_io(ch, iq, block, M, S)
        if args.full and world == 1 and not args.no_cpu_baseline:
            # headline: ~16 s incl. one stream per core; sub-records: the single-core and one-channel figures only (~6 s each)
            rec["cpu_baseline"] = cpu_baseline(fs, M, 8.0 if headline else 4.0, multi=headline)
    ch.close()
    iq.free()
    for b in pcm_bufs:
        b.free()
    if rec is None and par is not None:
        rec = {"parity_checked": {"all_ok": par["all_ok"]}}          # ranks > 0: only what decides the exit code
    return rec


def host_io(ch, iq, block, M, S):
    """PCIe-inclusive rates of the host-buffer entry points (host cf32 in, host int16 out), never the headline value:
    the synchronous call from pageable / pinned memory, and the asynchronous submit / collect pair (pinned, PIPE_DEPTH blocks in
    flight).  Pinned memory comes from the LIBRARY's HIP runtime (pmr_host_alloc); a torch.pin_memory() buffer is pinned in
    torch's own bundled runtime and reads as slow uncached pageable memory from here."""
    import ctypes
    import numpy as np
    nb = min(block, 1 << 22)                                     # 2^22 samples per call
    L = ch._L
    res = {}
    ns_c = ctypes.c_uint(0)
    x_host = iq.download(np.complex64, nb)
    pcm = np.zeros((M, S), dtype=np.int16)
    depth = L.pmr_chain_max_in_flight(ch.h)
    pinned = [ch.pinned_array(nb) for _ in range(depth)]
    for p in pinned:
        p[:] = x_host
    ch.reset()
    for kind, xin in (("sync_pageable", x_host), ("sync_pinned", pinned[0])):
        def host_call():
            rc = L.pmr_chain_process_block(ch.h, xin.ctypes.data, nb, pcm.ctypes.data, S, ctypes.byref(ns_c), None, None)
            assert rc == 0, rc
        host_call()
        t0 = time.perf_counter()
        for _ in range(8):
            host_call()
        res[kind] = 8 * nb / (time.perf_counter() - t0) / 1e6
    n_it = 24

    def async_rate(bufs, code):
        """submit / collect with `depth` blocks in flight; the first pass is a warm-up (the first blocks through the copy
        stream and the slots run at half speed: 2.8 vs 6.3 GS/s at 2^20-sample blocks, tools/async_sweep.py)"""
        rate = 0.0
        for timed in (False, True):
            ch.reset()
            for i in range(depth):
                assert L.pmr_chain_submit_block_fmt(ch.h, bufs[i].ctypes.data, code, nb, 1) == 0
            t0 = time.perf_counter()
            for i in range(n_it):
                assert L.pmr_chain_collect_block(ch.h, pcm.ctypes.data, None, S, ctypes.byref(ns_c), None, None) == 0
                assert L.pmr_chain_submit_block_fmt(ch.h, bufs[i % depth].ctypes.data, code, nb, 1) == 0
            dt = time.perf_counter() - t0
            for i in range(depth):
                assert L.pmr_chain_collect_block(ch.h, pcm.ctypes.data, None, S, ctypes.byref(ns_c), None, None) == 0
            rate = n_it * nb / dt / 1e6
        return rate

    res["async_pinned"] = async_rate(pinned, 0)
    # the receiver's own sample formats (include/pmr_io.h), converted on the device: 4 / 2 bytes per sample on the host link
    for name, code, dt_np in (("async_pinned_cs16", 1, np.int16), ("async_pinned_cu8", 2, np.uint8)):
        raws = [ch.pinned_array(2 * nb, dt_np) for _ in range(depth)]
        xi = np.empty(2 * nb, np.float32); xi[0::2] = x_host.real; xi[1::2] = x_host.imag
        for r in raws:
            r[:] = (np.clip(np.round(xi * 32768.0), -32768, 32767).astype(np.int16) if code == 1
                    else np.clip(np.round(xi * 127.5 + 127.5), 0, 255).astype(np.uint8))
        res[name] = async_rate(raws, code)
    return {"unit": "Msamples/s", "block_samples": nb, **res,
            "h2d_gbytes_per_s_async": res["async_pinned"] * 8 / 1e3,
            "note": "sync_*: pmr_chain_process_block (H2D + chain + D2H per call, nothing overlaps); async_pinned: "
                    "pmr_chain_submit_block / _collect_block with %d blocks in flight.  cf32 input is 8 B/sample: PCIe Gen5 x16 "
                    "(63 GB/s spec) caps any host-fed rate at ~7.9 GS/s" % depth}


def library_record(loaded=None):
    """The library this process runs on: path, sha256 of the file, sha256 of the sources that decide its traffic
    (build.kernel_sources_sha256), whether it reports an experiment build, and every PMR_* variable of the environment."""
    from sdr_pmr446_amd import build as _b
    alt = os.environ.get("PMR_LIBRARY")
    path = alt if alt else _b.LIB
    rec = {"path": os.path.relpath(path, ROOT) if os.path.abspath(path).startswith(ROOT) else path,
           "selected_by_PMR_LIBRARY": bool(alt), "sha256": None, "experiment_build": None,
           "kernel_sources_sha256": _b.kernel_sources_sha256(),
           "env": {k: v for k, v in sorted(os.environ.items()) if k.startswith("PMR_")}}
    try:
        rec["sha256"] = _b.library_sha256(path)
        if loaded is not None:                                               # (the library is loaded by chain.load(), after torch: see there)
            rec["experiment_build"] = bool(loaded.pmr_chain_info(None, 11, 0))       # PMR_INFO_EXPERIMENT_BUILD
    except Exception as e:
        rec["error"] = repr(e)[:200]
    return rec


def refuse_unless_product(lib_rec, args):
    if (lib_rec["selected_by_PMR_LIBRARY"] or lib_rec["experiment_build"]) and not args.allow_experiment:
        raise SystemExit("bench.py: refusing to print a headline from %s (PMR_LIBRARY set: %s, experiment build: %s); A/B tools pass "
                         "--allow-experiment" % (lib_rec["path"], lib_rec["selected_by_PMR_LIBRARY"], lib_rec["experiment_build"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="blocks per timed region (three blocks are in flight: a region "
                    "pays one pipeline fill/drain of ~0.17 ms, 6 %% of a 20-step region)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: repeated regions, kernel events and roofline, "
                    "the other legs and workloads, the oracle parity check, the CPU baseline (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write the int16 PCM of the last one "
                    "(channels x frames) as float32 DIR/pcm.npy (pcm_rank<r>.npy for rank r > 0); %d MB at most in all, a fixed "
                    "seeded sample of a larger output" % (DUMP_BYTES >> 20))
    ap.add_argument("--workload", default=HEADLINE, choices=sorted(WORKLOADS))
    ap.add_argument("--also", default=None, help="--full: comma list of further workloads reported as sub-records "
                                                 "(default at N = 1 with the default workload: cfg2,cfg3; 'none' disables)")
    ap.add_argument("--regions", type=int, default=None, help="how often the timed K-step region is repeated (default 1, "
                                                              "25 with --full)")
    ap.add_argument("--parity-blocks", type=int, default=4, help="--full: blocks of the un-synchronised oracle check (0 = skip)")
    ap.add_argument("--log2-block", type=int, default=None)
    ap.add_argument("--rotate", type=int, default=4, help="distinct device-resident blocks the timed steps rotate through (a power "
                    "of two; 1 = one block re-read every step)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-one-open", action="store_true", help="--full: skip the one-open-channel leg (profile runs: one kernel mix per trace)")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL) for real runs (falls back to gloo, and says so, if the "
                                                          "RCCL group does not come up); gloo lets two ranks share one GPU to "
                                                          "exercise the N > 1 code path on a 1-GPU box")
    ap.add_argument("--force-rccl", action="store_true", help="TEST ONLY: try the RCCL group even when ranks share a device (it must "
                    "fail there and the ranks must agree to fall back to gloo: the failure path of multigpu.init_dist, exercised on a 1-GPU box)")
    ap.add_argument("--host-io", action="store_true", help="(default since round 5; kept so that older command lines still parse)")
    ap.add_argument("--no-host-io", action="store_true",
                    help="--full: skip the PCIe-inclusive leg of the headline (host-buffer entry points on 2^22-sample calls, ~1 s)")
    ap.add_argument("--no-kernel-events", action="store_true", help="--full: skip per-kernel HIP events in the timed region")
    ap.add_argument("--ctcss", action="store_true", help="run with the CTCSS detector enabled (SURVEY s8 row f2) -- an A/B aid, "
                                                         "not the headline workload (the one_open_channel sub-record then is "
                                                         "the reference's mode: detector on the open channel only, :893)")
    ap.add_argument("--test-fail-rank", type=int, default=-1, help="TEST ONLY (--full): this rank falsifies the PCM it hands to its own oracle check, so "
                    "the job must print rank 0's line with that rank's verdict false and exit non-zero (tests/test_gpu_bench_ranks.py)")
    ap.add_argument("--allow-experiment", action="store_true", help="A/B tooling only: run on a library selected by PMR_LIBRARY or compiled with "
                    "-DPMR_EXPERIMENT; the line is then labelled as NOT a headline (metric prefixed, \"experiment\": true)")
    args = ap.parse_args()
    if args.regions is None:
        args.regions = 25 if args.full else 1

    # Which binary produces this line?  The headline is only ever taken from the in-tree product build: a library selected by
    # PMR_LIBRARY, or one compiled with the experiment gate open (csrc/pmr_experiment.h: timing-only hooks with wrong results), is
    # refused unless the caller says it is an A/B run -- and then the line says so.
    refuse_unless_product(library_record(), args)                        # PMR_LIBRARY: known before anything is loaded

    from sdr_pmr446_amd import multigpu

    rank, local_rank, world = multigpu.env_world()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: this process (which has made NO GPU call) starts
        # `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>` as a child, relays rank 0's JSON line
        # (the child's stdout is ours) and its exit code
        sys.exit(multigpu.self_launch(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE = %d but --gpus %d" % (world, args.gpus))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product has no CPU path)")
    ndev = torch.cuda.device_count()
    if args.dist_backend != "nccl" or ndev < world:
        local_rank = local_rank % ndev                               # ranks may share a device (self-test on a 1-GPU box)
        if args.dist_backend == "nccl" and ndev < world and not args.force_rccl:
            args.dist_backend = "gloo"                               # RCCL needs one device per rank
    torch.cuda.set_device(local_rank)
    from sdr_pmr446_amd import chain as _pmr
    lib_rec = library_record(_pmr.load())                                # ... the experiment gate: asked of the loaded library itself
    refuse_unless_product(lib_rec, args)
    dev = torch.device("cuda", local_rank)
    affinity = multigpu.bind_to_gpu_numa(local_rank, min(world, ndev)) if world > 1 else None
    dist = multigpu.init_dist(args.dist_backend, dev)

    if not args.full:
        also = []
    elif args.also is None:
        # N = 1: cfg2 and cfg3 ride along.  N > 1: cfg3 on every GPU IS BASELINE.json configs[3] ("cfg4": N independent
        # 61.44 MS/s streams, one per GPU) -- one timed region of it beside the headline
        also = [w for w in ("cfg2", "cfg3") if w != args.workload] if world == 1 else ["cfg3"]
        if args.workload != HEADLINE:
            also = []
    else:
        also = [w for w in args.also.split(",") if w in WORKLOADS and w != args.workload]

    head = measure(args.workload, args, rank, local_rank, world, dist, dev, headline=True, dump=args.dump_outputs)
    subs = {}
    for w in also:
        r = measure(w, args, rank, local_rank, world, dist, dev, headline=False)
        if r is not None:
            subs[w] = r
    # a parity failure on ANY rank fails the job (every rank knows: the verdicts were all-reduced), after the line is out
    parity_ok = all((r or {}).get("parity_checked", {}).get("all_ok", True) for r in [head] + list(subs.values()))
    if rank == 0:
        not_headline = lib_rec["selected_by_PMR_LIBRARY"] or lib_rec["experiment_build"]
        out = {"metric": ("EXPERIMENT BUILD, NOT A HEADLINE: " if not_headline else "") +
                         "complex-IQ Msamples/s through full channelize+demod chain", "value": head["value"],
               "unit": "Msamples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32", "data": "synthetic", "library": lib_rec}
        if not_headline:
            out["experiment"] = True
        if world > 1:
            out["dist"] = {"backend": args.dist_backend, "backend_used": dist.backend_used, "fallback_reason": dist.note,
                           "devices_visible": ndev, "rank0_affinity": affinity,
                           "use": "start/stop barrier and MAX of the elapsed time only (+ the AND of the ranks' parity verdicts): one "
                                  "independent IQ stream per rank, no data-path collective"}
        for k in ("timed_regions", "config", "roofline", "one_open_channel", "parity_checked", "host_io", "cpu_baseline"):
            if k in head:
                out[k] = head[k]
        if subs:
            out["also"] = subs
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy()
    if not parity_ok:
        sys.stderr.write("bench.py: PARITY FAILED on at least one rank (parity_checked.per_rank)\n")
        sys.exit(1)


if __name__ == "__main__":
    main()

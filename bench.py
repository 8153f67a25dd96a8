#!/usr/bin/env python3
"""bench.py -- headline benchmark of the raster hot path on MI355X.

A "step" is one frame of the hot path over one batch of synthetic input: ClearDepth + ClearColor +
one Rasterizer.RenderMesh per mesh (vertex transform, near clip, setup, 16x16-tile edge-function
rasterisation, depth test, nearest-texture Lambert+fog shading, blend, framebuffer write), flushed
and completed on the GPU.  Meshes and the texture are resident in HBM before the timed region.

Workload at N=1 (BASELINE.json configs[2], the configuration the metric is quoted on):
4096x4096, 1M triangles in 16 u16-indexed meshes, one 2048^2 RGBA8 texture, program
DUST2_LAMBERT_FOG (= Renderer.cs:830-860), CullMode.Back, DepthTest.LessEqual, BlendMode.Alpha.
At N>1 the same frame is sharded by tile rows (one band per rank, no collective while rendering)
and the colour bands are gathered to rank 0 over RCCL each step: strong scaling.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times --steps frames, writes
the last frame with --dump-outputs DIR and prints the line; --full adds what takes runs of its own: hipEvents in the timed region,
the one-stream kernel pass and stage breakdown behind it (`roofline`, `ms_per_step_unpipelined`) and the CPU baseline
(`cpu_baseline`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
HBM_MEASURED_GBS = 6290.0
BYTES_PER_WRITTEN_FRAGMENT = 20  # 16 B float4 colour + 4 B float depth
DUMP_MAX_BYTES = 64 << 20        # --dump-outputs: frames up to this size in all are written whole ...
DUMP_SAMPLE_PIXELS = 1 << 20     # ... larger ones as this many pixel positions, drawn once with a fixed seed
DUMP_SEED = 12345


def build_scene(name, args):
    from softwarerenderer_amd import scenes
    if name == "cfg3":
        return scenes.cfg3(bilinear=bool(getattr(args, "bilinear", False)))
    if name == "cfg4":
        return scenes.cfg4()
    if name == "cfg5":
        return scenes.cfg5()
    if name == "cfg2":
        return scenes.cfg2()
    if name == "cfg3_small":      # quick functional check of the bench itself
        return scenes.cfg3(1024, 1024, (4, 4), (64, 32), tex_size=512)
    raise SystemExit(f"unknown config {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--prime", type=int, default=32, help="untimed setup frames before warmup (runtime/buffer initialisation)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: hipEvents around the raster kernel in the timed region, a "
                         "one-stream pass and a per-stage breakdown behind it (roofline, ms_per_step_unpipelined) and, at N=1, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the frame of the last step as DIR/<name>.npy (float32): colour and depth at N=1, "
                         "rank 0's gathered colour at N>1; whole if at most 64 MB, else a fixed seeded sample of pixels (+ pixel_index)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--bilinear", action="store_true",
                    help="cfg3 through the BUILD-DEFINED bilinear texture filter (4 texel gathers per fragment) instead of the reference's "
                         "nearest filter (Texture.cs:43-63); parity is against the build's own oracle definition only")
    ap.add_argument("--fake-world", type=int, default=0,
                    help="self-test of the N>1 code path in ONE process: act as rank 0 of N, collectives stubbed (numbers are meaningless)")
    ap.add_argument("--no-profile-events", action="store_true", help="--full without hipEvents around kernels (and without the passes behind the timed region)")
    ap.add_argument("--gather", choices=["rgb32f", "rgba32f", "p2p"], default="rgb32f",
                    help="N>1: what reaches rank 0 per frame and how -- rgb32f = the present payload of MainWindow.OnRender "
                         "(Vector4 -> Vector3 flatten, 12 B/pixel) by an RCCL gather, rgba32f = the raw colour buffer (16 B/pixel) "
                         "by an RCCL gather, p2p = the rgb32f payload stored by every rank's flatten kernel straight into rank 0's "
                         "frame through a peer-mapped (IPC) pointer over xGMI: no collective in the data path; the ranks meet at a barrier "
                         "every 32 frames and at the ends of the warm-up / timed regions (checkpoint()), not per frame: between checkpoints "
                         "rank 0's frame is a landing zone that nobody reads")
    ap.add_argument("--stripes", type=int, default=0,
                    help="N>1: instead of one contiguous band per rank, interleave stripes of this many tile rows round-robin over "
                         "the ranks (swr_set_band_interleaved; load balance for clustered scenes).  RCCL gather modes only.")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend; gloo (control plane only, needs --gather p2p) rehearses the N>1 path with "
                         "several ranks on ONE GPU (SWR_BENCH_ONE_DEVICE=1), which RCCL refuses")
    ap.add_argument("--pipelining", type=int, choices=[0, 1, 2], default=1,
                    help="frames in flight inside the library (swr_set_pipelining): 1 (the library's default) = every frame's front end runs on a "
                         "second stream beside the previous frame's raster kernel, 0 = never (one stream), 2 = only frames of up to 2^15 tiles or "
                         "batches of up to 2^17 triangles")
    ap.add_argument("--camera-jitter", type=float, default=0.0,
                    help="perturb the view matrix of every frame on the host (a translation of this amplitude in view space plus a small "
                         "yaw, a different one each frame): the tile order feeds on the previous frame's fragment counts, this shows it is "
                         "not fitted to a repeated frame")
    ap.add_argument("--force-dist", action="store_true",
                    help="N=1 only: take the N>1 code path end to end with a world of ONE rank on the nccl (RCCL) backend -- "
                         "init_process_group, SetBand, two bound band buffers, async dist.gather, work.wait(), the all-reduced replay "
                         "flag on the GPU, record_stream, checkpoint / resend: the RCCL leg rehearsed on the one GPU of a test box")
    ap.add_argument("--print-src-hash", action="store_true", help="print the kernel-source hash (tools/profile_round.sh) and exit")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.print_src_hash:
        print(kernel_source_hash())
        return

    rc = launch_ranks_if_needed(args, sys.argv[1:])
    if rc is not None:
        raise SystemExit(rc)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world
    if args.force_dist and (world != 1 or args.fake_world > 1):
        raise SystemExit("--force-dist is the one-rank rehearsal of the N>1 path: use it with --gpus 1 and without --fake-world")
    if args.force_dist and args.gather == "p2p":
        raise SystemExit("--force-dist rehearses the RCCL gather modes (a process cannot open its own IPC handle): use rgb32f or rgba32f")
    dist_on = world > 1 or args.force_dist          # the multi-GPU code path (bands, band buffers, gather, checkpoints)
    profile = args.full and not args.no_profile_events

    import torch                      # plumbing: device memory for the bands, streams, RCCL
    import torch.distributed as dist
    if args.fake_world > 1 and world == 1:
        class _FakeDist:                       # rank 0 of N without peers: exercises bands, double buffering, bookkeeping
            class ReduceOp: SUM = 0; MAX = 1
            def barrier(self): pass
            def all_reduce(self, t, op=None): pass
            class _Work:
                def wait(self): return True
            def gather(self, t, gather_list=None, dst=0, group=None, async_op=False):
                if gather_list is not None:
                    gather_list[0].copy_(t[:gather_list[0].shape[0]])
                return self._Work() if async_op else None
            def destroy_process_group(self): pass
        dist = _FakeDist()
        world = args.fake_world
        args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    if os.environ.get("SWR_BENCH_ONE_DEVICE", "0") == "1":
        local_rank = 0                    # rehearsal: every rank on GPU 0 (at most 6 processes may share a card on this pool)
    torch.cuda.set_device(local_rank)
    if args.force_dist:
        import socket
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", local_rank))
    if world > 1 and not args.fake_world:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "gloo":
            if args.gather != "p2p":
                raise SystemExit("--backend gloo carries no GPU payload: use it with --gather p2p")
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import numpy as np
    from softwarerenderer_amd import Device, MainWindow, multigpu, scenes

    scene = build_scene(args.config, args)
    W, H = scene.width, scene.height
    dev = Device(local_rank)
    dev.set_pipelining(args.pipelining)
    window = MainWindow(dev, W, H)
    color_t = depth_t = None
    overlap = dist_on and os.environ.get("SWR_BENCH_OVERLAP", "1") != "0"
    if dist_on:
        band = multigpu.band_partition(H, world)[rank]
        rows = multigpu.max_band_rows(H, world)
        if args.stripes > 0:
            if args.gather == "p2p":
                raise SystemExit("--stripes needs an RCCL gather mode (a stripe set is not one contiguous block of rank 0's frame)")
            rows = max(len(r) for r in multigpu.stripe_rows(H, world, args.stripes))
        # two band buffers: the colour gather of frame i (RCCL, xGMI) overlaps the rendering of frame i+1
        color_t = [torch.zeros((rows, W, 4), dtype=torch.float32, device="cuda") for _ in range(2 if overlap else 1)]
        depth_t = [torch.zeros((rows, W), dtype=torch.float32, device="cuda") for _ in range(2 if overlap else 1)]
        if args.stripes > 0:
            window.SetBandInterleaved(rank, world, args.stripes)
        else:
            window.SetBand(*band)
        window.BindFramebuffer(color_t[0].data_ptr(), depth_t[0].data_ptr())
    p2p = dist_on and args.gather == "p2p"
    rgb = dist_on and args.gather in ("rgb32f", "p2p")
    chan = 3 if rgb else 4
    rgb_t = [torch.zeros((rows, W, 3), dtype=torch.float32, device="cuda") for _ in range(len(color_t))] if (rgb and not p2p) else None
    frame_t = torch.empty((H, W, chan), dtype=torch.float32, device="cuda") if (dist_on and rank == 0) else None
    peer_rows = None
    if dist_on:
        # render, flatten and the consumer of the band run in stream order on torch's current stream: no host round trip
        # between a frame's last kernel and its gather (optimistic flushes are validated later, see validate_previous)
        # (a stream of its own: torch's default stream is the NULL stream, which swr_set_stream reads as "context's own")
        side = torch.cuda.Stream()
        torch.cuda.set_stream(side)
        dev.set_stream(side.cuda_stream)
    if p2p:
        # rank 0 shares its frame (one IPC handle, exchanged once); every rank maps it and its flatten kernel stores the
        # band's rows directly into it over xGMI
        from torch.multiprocessing.reductions import reduce_tensor
        box = [reduce_tensor(frame_t) if rank == 0 else None]
        if not args.fake_world:
            dist.broadcast_object_list(box, src=0)
        if rank == 0:
            peer_frame = frame_t
        else:
            fn, fargs = box[0]
            peer_frame = fn(*fargs)                        # hipIpcOpenMemHandle (lazy peer access) inside torch
        y0, nrows = multigpu.band_pixel_rows(H, band)
        peer_rows = peer_frame[y0:y0 + nrows]              # contiguous rows of rank 0's frame = this rank's band
    renderer = scenes.SceneRenderer(dev, scene, window=window)
    state = {"i": 0, "works": [None] * (len(color_t) if color_t else 1), "ev": [], "since_check": 0,
             "replays": dev.replay_count() if dist_on else 0, "resent": 0, "last_k": None, "frame_no": 0}
    xfer = torch.cuda.Stream() if dist_on else None      # rank 0: post-collective assembly (stripes / unequal bands), off the render stream
    stripe_bufs = None

    def send_band(k):
        """flatten (on the GPU) + hand the band of buffer k to rank 0, stream-ordered behind the frame's kernels and WITHOUT making
        the render stream wait for the transfer; returns the collective's handle (None for p2p)"""
        nonlocal stripe_bufs
        if p2p:
            window.FlattenToAsync(peer_rows.data_ptr())     # the kernel's stores ARE the transfer (peer-mapped pointer over xGMI)
            return None
        if rgb:
            window.FlattenToAsync(rgb_t[k].data_ptr())     # present payload: Vector4 -> Vector3 on the GPU (MainWindow.cs:234-240)
        payload = rgb_t[k] if rgb else color_t[k]
        if args.stripes > 0:
            # stripes: gather the per-rank stripe buffers, then one indexed row copy per rank scatters them into the frame
            if rank == 0 and stripe_bufs is None:
                stripe_bufs = [[torch.empty_like(payload) for _ in range(world)] for _ in range(len(color_t))]
            w = dist.gather(payload, gather_list=stripe_bufs[k] if rank == 0 else None, dst=0, async_op=True)
            if rank == 0:
                with torch.cuda.stream(xfer):
                    w.wait()
                    multigpu.assemble_stripes(stripe_bufs[k], H, world, args.stripes, frame=frame_t)
            return w
        return multigpu.gather_bands(payload, H, W, rank, world, dst=0, frame=frame_t, dist=dist, async_op=True, post_stream=xfer,
                                     force_collective=args.force_dist)[1]

    def before_reuse(k):
        """buffer k was last used two frames ago: its transfer must be over before the next frame renders into it.  A stream-level
        wait (RCCL work handle / the assembly stream): the host does not block, the GPU runs back to back."""
        w = state["works"][k]
        if w is not None:
            w.wait()
            state["works"][k] = None
        if xfer is not None and rank == 0:
            torch.cuda.current_stream().wait_stream(xfer)

    def checkpoint():
        """Every few frames and at every barrier: drain, confirm across ranks that all stores / collectives are complete, and let the
        backend look at its optimistic batches (swr_sync validates and replays).  A replay (never in steady state) means the payload
        of the frames sent since is stale: the last one is sent again."""
        for k in range(len(state["works"])):
            before_reuse(k)
        torch.cuda.current_stream().synchronize()
        if xfer is not None:
            xfer.synchronize()
        if dist_on and not args.fake_world:
            dist.barrier()
        dev.sync()
        r = dev.replay_count()
        replayed = dist_on and r != state["replays"]
        state["replays"] = r
        if dist_on and not args.fake_world:
            # the re-send below is a collective in the RCCL modes and a store into rank 0's frame in p2p mode: every rank has to
            # know whether ANY rank replayed, take part, and meet again before rank 0 may read its frame
            flag = torch.tensor([1 if replayed else 0], dtype=torch.int32, device="cpu" if args.backend == "gloo" else "cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            replayed = bool(flag.item())
        if replayed and state["last_k"] is not None:
            k = state["last_k"]
            window.BindFramebuffer(color_t[k].data_ptr(), depth_t[k].data_ptr())
            w = send_band(k)
            if w is not None:
                w.wait()
            torch.cuda.current_stream().synchronize()
            if xfer is not None:
                xfer.synchronize()
            state["resent"] += 1
            if not args.fake_world:
                dist.barrier()
        state["since_check"] = 0

    def barrier():
        checkpoint()
        torch.cuda.synchronize()

    def step():
        if args.camera_jitter > 0.0:
            renderer.jitter_views(state["frame_no"], args.camera_jitter)
        state["frame_no"] += 1
        if not dist_on:
            renderer.submit_frame()
            dev.flush()
            return
        k = state["i"] % len(color_t)
        state["i"] += 1
        before_reuse(k)
        if len(color_t) > 1:
            window.BindFramebuffer(color_t[k].data_ptr(), depth_t[k].data_ptr())     # no host wait (a batch remembers its target)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        renderer.submit_frame()
        dev.flush()
        e1.record()                                         # render leg of this rank, on the stream the kernels run on
        state["ev"].append((e0, e1))
        state["works"][k] = send_band(k)                    # the transfer of frame i overlaps the rendering of frame i+1
        state["last_k"] = k
        if not overlap:
            before_reuse(k)
        state["since_check"] += 1
        if state["since_check"] >= 32:
            checkpoint()

    # Setup (untimed, not part of warmup): the first frame sizes the pair buffers synchronously, and the HIP runtime
    # that torch bundles spends a one-off ~45 ms around its 16th submission growing
    # internal pools.  Prime past both so that the W warmup + K timed steps see the steady state.
    t_prime = time.perf_counter()
    n_prime = 0
    # (the count must be the same on every rank: only a single process may extend it by wall time)
    while n_prime < args.prime or (not dist_on and time.perf_counter() - t_prime < 0.2 and n_prime < 10 * args.prime):
        step()
        dev.sync()
        n_prime += 1
    barrier()
    # ... and with frames in flight the runtime grows the pools of the SECOND stream (and of the cross-stream events) only once the
    # queues run deep, i.e. when frames follow each other without a synchronisation: one untimed back-to-back burst does that here
    # (without it the first ~25 pipelined frames of a process contain a one-off stall of several milliseconds)
    for _ in range(max(args.prime, 1) if args.pipelining else 0):
        step()
    barrier()
    # the prime may run longer by wall time: a camera-jitter sequence restarts here, so the timed frames are the same in every run
    state["frame_no"] = 0
    for _ in range(args.warmup):
        step()
    barrier()
    dev.reset_stats()
    if profile:
        dev.profile_reset()
        # hipEvents around the dominant kernel, on the stream it is launched on: on EVERY launch of a short timed region (the driver's
        # 20 steps: a mean of 5 samples moved by 7 % between two passes of one run), on every 4th launch of a long one (an event pair
        # costs ~10 us of stream time)
        dev.profile_enable(2 if args.steps <= 32 else 3)
    barrier()
    state["ev"] = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    render_s = 1e-3 * sum(a.elapsed_time(b) for a, b in state["ev"]) if dist_on else 0.0
    prof = dev.profile() if profile else None
    samples = np.sort(dev.raster_samples()) if profile else None
    st = dev.stats()
    if args.dump_outputs and rank == 0:
        if dist_on:
            frames = {"color": frame_t.cpu().numpy()}                 # what rank 0 holds: the gathered frame
        else:
            color, depth = window._read(True, True)                     # what SceneRenderer.render() hands its caller
            frames = {"color": color, "depth": depth}
        dump_outputs(args.dump_outputs, frames, np)
    stage_ms = None
    isolated = None
    if profile:
        # OUTSIDE the timed region, frames NOT in flight (one stream: a kernel has the chip to itself, which is what a kernel's
        # roofline is quoted on): (1) the raster kernel of every launch of as many frames as were timed, and the frame time,
        # (2) a per-stage breakdown from a few frames with events around every stage
        dev.set_pipelining(0)
        n_iso = max(8, min(args.steps, 64))
        for _ in range(3):
            step()
        barrier()
        dev.profile_reset(); dev.profile_enable(2)
        t_iso = time.perf_counter()
        for _ in range(n_iso):
            step()
        barrier()
        t_iso = time.perf_counter() - t_iso
        iso = np.sort(dev.raster_samples())
        if iso.size:
            isolated = {"raster_ms_median": round(float(np.median(iso)), 4), "raster_ms_min": round(float(iso[0]), 4),
                        "raster_ms_max": round(float(iso[-1]), 4), "launches": int(iso.size),
                        "ms_per_step_unpipelined": round(1e3 * t_iso / n_iso, 4)}
        dev.profile_enable(1)
        for _ in range(3):
            step()
        barrier()
        dev.profile_reset()
        n_extra = 20
        for _ in range(n_extra):
            step()
        barrier()
        p2 = dev.profile()
        stage_ms = {k: round(p2[k] / n_extra, 4) for k in
                    ("vertex_ms", "setup_ms", "bin_ms", "sort_ms", "cover_ms", "raster_ms", "clear_ms", "total_ms")}
        dev.profile_enable(0)
        dev.set_pipelining(args.pipelining)

    # whole-job numbers: max time over ranks, fragments summed over ranks
    red_dev = "cpu" if (dist_on and args.backend == "gloo" and not args.fake_world) else "cuda"
    counts = torch.tensor([st["fragments_tested"], st["fragments_written"], st["tile_pairs"]], dtype=torch.float64, device=red_dev)
    tmax = torch.tensor([elapsed, render_s], dtype=torch.float64, device=red_dev)
    if dist_on:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax[0].item())
    render_s = float(tmax[1].item())
    frags_tested = counts[0].item() / args.steps
    frags_written = counts[1].item() / args.steps
    n_tris = scene.n_triangles

    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        out = {
            "metric": "Mfragments/s (depth-tested + textured fragments, whole frame)",
            "value": round(frags_tested / (ms_per_step * 1e-3) / 1e6, 3),
            "unit": "Mfragments/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{args.config}: {W}x{H}, {n_tris} triangles in {len(scene.draws)} u16 meshes, "
                                   f"{('2048^2 RGBA8 ' + ('bilinear (build-defined) ' if scene.bilinear else 'nearest ') + 'texture, ') if scene.textures else ''}"
                                   f"program {scene.draws[0].program.name}, {scene.draws[0].cull.name}/"
                                   f"{scene.draws[0].depth_test.name}/{scene.draws[0].blend.name}",
                       "pipelining": args.pipelining, "camera_jitter": args.camera_jitter,
                       "parallelism": "1 GPU" if not dist_on else (f"{world} tile-row bands + RCCL gather of the {args.gather} frame to rank 0" if not p2p else
                                      f"{world} tile-row bands, each rank's flatten kernel stores its rgb32f band into rank 0's frame through a peer-mapped pointer (xGMI), barrier every 32 frames")
                                      + (" (gather of frame i overlaps rendering of frame i+1)" if overlap else "")
                                      + f"; gather_payload={args.gather}, {4 * chan} B/pixel",
                       "gather_payload": None if not dist_on else args.gather,
                       "gather_bytes_per_pixel": None if not dist_on else 4 * chan},
            "mtriangles_per_s": round(n_tris / (ms_per_step * 1e-3) / 1e6, 3),
            "fragments_tested_per_frame": int(frags_tested),
            "fragments_written_per_frame": int(frags_written),
            "tile_pairs_per_frame": int(counts[2].item() / args.steps),
            "device": dev.name,
        }
        if dist_on:
            # the two legs of a multi-GPU step: rendering the bands (slowest rank, wall time until its band is final)
            # and the xGMI gather of the frame into rank 0, which overlaps the next frame's rendering
            out["multi_gpu"] = {"render_ms_per_step": round(1e3 * render_s / args.steps, 4),
                                "gather_payload": args.gather, "frames_resent_after_replay": state["resent"],
                                "gather_mb_per_frame_into_rank0": round(H * W * chan * 4 * (world - 1) / world / 1e6, 1),
                                "forced_one_rank_rehearsal": bool(args.force_dist),
                                "model": multi_gpu_model(args.config, world, H, W, chan)}
        if prof is not None and prof["raster_launches"] > 0 and samples is not None and samples.size:
            # dominant kernel = k_raster_c; algorithmic bytes = 20 B per WRITTEN fragment (rank 0's band at N>1).  With frames in flight
            # the kernel shares the chip with the NEXT frame's front end during the timed region, and a roofline is a statement about a
            # kernel that has the chip: `kernel_ms` / `achieved` / `frac` are therefore the median of the per-launch hipEvent samples of
            # the one-stream pass that follows the timed region in this same process (same frames, same launch count; rocprofv3's
            # "alone" launches, profiles/*_summary.md), and the timed region's own samples ride along as `timed_region` (rocprofv3's
            # "beside a front end" launches).  Without pipelining the two are the same measurement twice and must agree within 3 %.
            timed_ms = float(np.median(samples))
            raster_ms = isolated["raster_ms_median"] if isolated is not None else timed_ms
            written_local = st["fragments_written"] / args.steps
            achieved = written_local * BYTES_PER_WRITTEN_FRAGMENT / (raster_ms * 1e-3) / 1e9
            frame_bytes = (W * H if not dist_on else color_t[0].shape[0] * W) * 20.0
            # (the committed PMC passes are of the nearest-filter frame: the bilinear one has no traffic figure)
            traffic, traffic_detail = pmc_traffic(args.config, world) if not getattr(args, "bilinear", False) else (None, None)
            out["roofline"] = {
                "bound": "hbm", "kernel": "k_raster_c",
                "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5),
                "frac_of_measured_copy_peak": round(achieved / HBM_MEASURED_GBS, 5),
                "traffic": traffic, "traffic_detail": traffic_detail,
                "traffic_unit": "GB per launch = 2 x FETCH_SIZE + WRITE_SIZE of the committed PMC passes of this build (null: none for this build); algorithmic = written fragments x 20 B",
                "algorithmic_gb_per_launch": round(written_local * BYTES_PER_WRITTEN_FRAGMENT / 1e9, 4),
                "kernel_ms": round(raster_ms, 4),
                "kernel_ms_source": ("one-stream pass behind the timed region (pipelining off: the kernel alone on the chip), hipEvent pair on every launch, median"
                                     if isolated is not None else "timed region, hipEvent pairs, median"),
                "frame_level_frac": round(frame_bytes / (raster_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                "kernel_launches_timed": int(samples.size),          # launches of the timed region that carried an event pair (all, up to 32 steps)
                "timed_region": {
                    "kernel_ms_median": round(timed_ms, 4), "kernel_ms_min": round(float(samples[0]), 4), "kernel_ms_max": round(float(samples[-1]), 4),
                    "kernel_ms_mean": round(prof["raster_ms"] / prof["raster_launches"], 4),
                    "kernel_launches_timed": int(samples.size),      # every launch of a timed region of <= 32 steps, else every 4th
                    "frac": round(written_local * BYTES_PER_WRITTEN_FRAGMENT / (timed_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                    "note": ("frames in flight: the kernel runs beside the next frame's front end (longer launch, shorter frame)" if args.pipelining
                             else "one stream: the same measurement as kernel_ms"),
                },
                "stage_ms_per_step": stage_ms,
                "stage_note": "20 frames on one stream with an event pair around EVERY stage: a breakdown, not a timing -- back-to-back event records "
                              "before a kernel lengthen it (raster: +5-8 % against kernel_ms, which has the pair on that kernel alone)",
            }
            if isolated is not None:
                out["roofline"]["kernel_ms_isolated"] = raster_ms            # (= kernel_ms; kept under the name round 3's verdict asked for)
                out["roofline"]["kernel_ms_median"] = raster_ms
                out["roofline"]["kernel_ms_min"] = isolated["raster_ms_min"]
                out["roofline"]["kernel_ms_max"] = isolated["raster_ms_max"]
                out["roofline"]["kernel_launches"] = isolated["launches"]
                rel = abs(timed_ms - raster_ms) / raster_ms
                if rel > 0.03:
                    out["roofline"]["warning"] = (f"the timed region's kernel samples and the one-stream kernel_ms differ by {100 * rel:.1f} %"
                                                  + (": expected with frames in flight (the kernel shares the chip with the next frame's front end)"
                                                     if args.pipelining else ": measurement noise above 3 %"))
            vf = valu_floor(args.config, world, raster_ms, written_local) if not getattr(args, "bilinear", False) else None
            if vf is not None:
                out["roofline"]["valu_floor"] = vf
        if isolated is not None:
            out["ms_per_step_unpipelined"] = isolated["ms_per_step_unpipelined"]
        if args.full and not dist_on and not args.no_cpu_baseline:
            renderer.jitter_views(0, 0.0)              # the comparison frame is the unperturbed one
            out["cpu_baseline"] = cpu_baseline(scene, renderer, np)
        print(json.dumps(out), flush=True)

    if rank == 0 and dist_on and os.environ.get("SWR_BENCH_DUMP_FRAME"):     # tests: the frame rank 0 holds after the last step
        np.save(os.environ["SWR_BENCH_DUMP_FRAME"], frame_t.cpu().numpy())
    renderer.close()
    dev.close()
    if dist_on and not args.fake_world:
        dist.destroy_process_group()


def dump_outputs(out_dir, frames, np):
    """--dump-outputs: `frames` (name -> float32 array of H x W [x C]) as out_dir/<name>.npy.  Whole when they hold at most
    DUMP_MAX_BYTES together; otherwise the same DUMP_SAMPLE_PIXELS pixel positions of each (seeded, sorted), as rows of
    <name>.npy, and their flat indices y * W + x as pixel_index.npy (float64, exact)."""
    os.makedirs(out_dir, exist_ok=True)
    if sum(a.nbytes for a in frames.values()) <= DUMP_MAX_BYTES:
        for name, a in frames.items():
            np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
        return
    h, w = next(iter(frames.values())).shape[:2]
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(h * w, min(DUMP_SAMPLE_PIXELS, h * w), replace=False))
    np.save(os.path.join(out_dir, "pixel_index.npy"), idx.astype(np.float64))
    for name, a in frames.items():
        rows = a.reshape(h * w, -1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(rows[:, 0] if a.ndim == 2 else rows, dtype=np.float32))


def launch_ranks_if_needed(args, argv, run=None):
    """`python bench.py --gpus N` started directly (no WORLD_SIZE in the environment): start the N ranks as FRESH child processes
    -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same arguments>` --
    forward what they print (rank 0's JSON line) and return their exit code.  This process has not imported torch or touched
    the GPU and never does (a process that has initialised HIP must not exec or fork workers on this pool); it only waits.
    Returns None when there is nothing to launch (N = 1, a --fake-world rehearsal, or already a rank of a launched job)."""
    if args.gpus <= 1 or args.fake_world > 1 or "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return None
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL / peer-mapped frames across processes need it on this pool
    env.setdefault("OMP_NUM_THREADS", "1")
    r = (run or subprocess.run)(cmd, env=env, cwd=ROOT)
    return int(r.returncode)


XGMI_LINK_GBS = 64.0            # one xGMI link, one direction, as RCCL send/recv sustains it (64-77 GB/s)


def multi_gpu_model(config, world, H, W, chan):
    """What DESIGN.md section 6 predicts for this N, printed next to what was measured so that a SCALE run can be read line by line:
    every rank runs the vertex + setup stages for ALL triangles and bins / sorts / covers / rasterises its band (1/N of the pairs);
    a rank's render leg is the sum of its stages scaled by the measured single-GPU frame / stage-sum ratio; all N-1 bands travel to rank 0 concurrently, one xGMI
    link each.  Stage times: the newest committed single-GPU line of this config (profiles/r*_bench_with_cpu.json); null if none."""
    import glob
    gather_ms = (H * W * chan * 4.0 / max(world, 1)) / (XGMI_LINK_GBS * 1e9) * 1e3 if world > 1 else 0.0
    out = {"link_gb_s": XGMI_LINK_GBS, "gather_ms": round(gather_ms, 4), "render_ms": None, "step_ms": None, "source": None}
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_final_bench_with_cpu.json")), reverse=True):
        try:
            j = json.load(open(path))
            stg = j["roofline"]["stage_ms_per_step"]
            if not j["config"]["workload"].startswith(config + ":"):
                continue
        except Exception:
            continue
        replicated = stg["vertex_ms"] + stg["setup_ms"]
        banded = stg["bin_ms"] + stg["sort_ms"] + stg["cover_ms"]
        front = replicated + banded / world
        raster = stg["raster_ms"] / world
        # frames in flight do NOT make the render leg max(front end, raster): the raster kernel's vector pipe is nearly saturated, so
        # what runs beside it takes from it what it gains (profiles/r04_frames_in_flight.md) -- the measured frame is the SUM of the
        # stage times scaled by what the overlap (and the absence of per-stage event pairs) bought on one GPU
        scale = j["ms_per_step"] / stg["total_ms"] if stg.get("total_ms") else 1.0
        render = (front + raster) * scale
        out.update({"render_ms": round(render, 4), "front_ms": round(front, 4), "raster_ms": round(raster, 4), "overlap_scale": round(scale, 4),
                    "step_ms": round(max(render, gather_ms), 4), "source": os.path.basename(path)})
        break
    return out


def kernel_source_hash():
    """sha256 over the kernel sources the library is built from: ties a committed PMC pass to the build it measured."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "softwarerenderer_amd", "csrc")
    for f in sorted(os.listdir(d)) + [os.path.join("..", "..", "include", "swr.h")]:
        path = os.path.join(d, f)
        if os.path.isfile(path):
            h.update(os.path.basename(f).encode()); h.update(open(path, "rb").read())
    return h.hexdigest()


def pmc_traffic(config, world):
    """HBM-side bytes per k_raster_c launch from the committed PMC passes of this same command (rocprofv3 --pmc FETCH_SIZE /
    --pmc WRITE_SIZE in separate passes; they cannot run inside bench.py).  Corrected as MI355X_MICROARCH.md prescribes: the
    counters are KiB, and gfx950's FETCH_SIZE tallies a 128-B request as 64 B, so the read side is doubled (an upper bound for this
    kernel's mix of 16-B gathers and 4-B texel gathers; the raw figure rides along).  The pass is only valid for the build it
    measured: the JSON carries a hash of the kernel sources, and a different build reports null instead of a stale number."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))
    if world != 1 or not cands:
        return None, None
    j = json.load(open(cands[-1]))
    t = j.get(config)
    if not t or j.get("csrc_sha256") != kernel_source_hash():
        return None, {"stale": os.path.basename(cands[-1])} if t else None
    raw = (t["fetch_kib_raw"] + t["write_kib"]) * 1024 / 1e9
    cor = (2.0 * t["fetch_kib_raw"] + t["write_kib"]) * 1024 / 1e9
    return round(cor, 4), {"file": os.path.basename(cands[-1]), "fetch_raw_gb": round(t["fetch_kib_raw"] * 1024 / 1e9, 4),
                           "write_gb": round(t["write_kib"] * 1024 / 1e9, 4), "raw_sum_gb": round(raw, 4)}


NUM_SIMDS = 1024               # MI355X: 256 CUs x 4 SIMD-32
VALU_ISSUE_CYCLES = 2          # a wave64 VALU instruction occupies a SIMD-32 for 2 cycles (MI355X_MICROARCH.md)
PEAK_CLOCK_GHZ = 2.4
REFERENCE_VALU_PER_64_FRAGMENTS = 215      # Interpolate + Renderer.FragmentShader + Blend, counted in the ISA: no
                                           # multiply-add of the reference may be fused, every division and square root is IEEE


def valu_floor(config, world, raster_ms, written_per_launch):
    """The issue-bound floor of the dominant kernel next to its HBM roofline (the gap is issue efficiency x instruction
    overhead, not bytes): wave-level VALU instructions per launch from the committed SQ pass of THIS build (same source-hash rule as
    pmc_traffic) x 2 cycles / 1024 SIMDs / clock.  `reference_only_ms` is the same arithmetic for the reference's own unfusable
    float work alone (215 VALU per 64 written fragments)."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))
    if world != 1 or not cands:
        return None
    j = json.load(open(cands[-1]))
    t = j.get(config)
    if not t or "valu_wave_insts" not in t or j.get("csrc_sha256") != kernel_source_hash():
        return None
    v = t["valu_wave_insts"]
    ms = v * VALU_ISSUE_CYCLES / NUM_SIMDS / (PEAK_CLOCK_GHZ * 1e9) * 1e3
    ref_ms = written_per_launch / 64.0 * REFERENCE_VALU_PER_64_FRAGMENTS * VALU_ISSUE_CYCLES / NUM_SIMDS / (PEAK_CLOCK_GHZ * 1e9) * 1e3
    out = {"valu_wave_insts_per_launch": v, "ms_at_full_issue": round(ms, 4), "issue_efficiency": round(ms / raster_ms, 4),
           "valu_per_64_written_fragments": round(v / (written_per_launch / 64.0), 1),
           "reference_only_valu_per_64_fragments": REFERENCE_VALU_PER_64_FRAGMENTS, "reference_only_ms": round(ref_ms, 4),
           "hbm_frac_if_issue_bound": round(written_per_launch * BYTES_PER_WRITTEN_FRAGMENT / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "unit": "wave64 VALU instructions x 2 cycles / 1024 SIMD-32 / 2.4 GHz",
           "other_wave_insts_per_launch": {k: t[k] for k in ("salu_wave_insts", "lds_wave_insts", "vmem_rd_wave_insts") if k in t}}
    if "wave_quad_cycles" in t and "wait_any_quad_cycles" in t:
        out["wave_time_in_s_waitcnt"] = round(t["wait_any_quad_cycles"] / t["wave_quad_cycles"], 4)
    return out


def cpu_baseline(scene, renderer, np):
    """The C restatement of the reference (oracle/, kind "port") timed on this box's host cores on the SAME frame:
    the threaded variant (persistent pool, a mutex per tile like Rasterizer.cs:478, Parallel.For-style chunks) at several
    thread counts -- 1 warm-up + 5 timed frames each, median -- with the fastest as `value` / `cores`, plus ONE serial frame
    (the oracle of record: `serial_value`), which is also compared word for word with the GPU frame.  Bounded: ~20 s."""
    from oracle.binding import OracleRenderer
    ncpu = os.cpu_count() or 1
    tried, best = {}, None
    budget_t0 = time.perf_counter()
    for threads in sorted({ncpu, max(1, ncpu // 2), min(ncpu, 64), min(ncpu, 32), min(ncpu, 16)}, reverse=True):
        o = OracleRenderer(scene.width, scene.height, threads=threads)
        o.render_scene(scene)                      # warm-up (also starts the pool)
        times = []
        for _ in range(5):
            o.reset_stats()
            t0 = time.perf_counter()
            o.render_scene(scene)
            times.append(time.perf_counter() - t0)
        st = o.stats()
        o.close()
        t = sorted(times)[len(times) // 2]
        tried[str(threads)] = round(st["fragments_tested"] / t / 1e6, 1)
        if best is None or t < best[0]:
            best = (t, threads, st, len(times))
        if time.perf_counter() - budget_t0 > 12.0:
            break
    t, cores, st, nrep = best
    res = {"value": round(st["fragments_tested"] / t / 1e6, 3), "unit": "Mfragments/s", "cores": cores, "kind": "port",
           "sample": f"the whole {scene.name} frame: median of {nrep} timed frames after 1 warm-up per thread count, fastest count reported "
                     f"(host has {ncpu} hardware threads); threaded C restatement of Rasterizer.cs (oracle/swr_oracle.c: persistent pool, "
                     f"per-tile mutexes, far-apart triangle chunks); serial_value = one frame on 1 thread",
           "ms_per_frame": round(t * 1e3, 2), "mfragments_per_s_by_threads": tried}
    # one serial frame = the oracle of record; doubles as a full-size parity check of the GPU frame
    o = OracleRenderer(scene.width, scene.height, threads=1)
    t0 = time.perf_counter()
    rc, rd = o.render_scene(scene)
    ts = time.perf_counter() - t0
    sst = o.stats()
    o.close()
    res["serial_value"] = round(sst["fragments_tested"] / ts / 1e6, 3)
    res["serial_ms_per_frame"] = round(ts * 1e3, 1)
    gc, gd = renderer.render()
    depth_exact = bool(np.array_equal(gd.view(np.uint32), rd.view(np.uint32)))
    a = gc.view(np.int32).astype(np.int64); b = rc.view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a); b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    res["gpu_frame_matches_serial_port"] = {"depth_bit_exact": depth_exact, "color_max_ulp": int(np.abs(a - b).max())}
    return res


if __name__ == "__main__":
    main()

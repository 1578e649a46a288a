"""An on-device wavefront path frame over the stage kernels (the shape of docs/src/wavefront-renderer.jl:185-600, without shading).

One frame: primary rays (generate_primary_rays_lookat!) -> closest_hit, then per depth b: shadow rays toward a point light -> any_hit,
and while b + 1 < depth: [hit compaction] -> diffuse bounce rays -> closest_hit.  Every stage runs on one stream, with no host
synchronisation and no parallel branches, so a frame can be captured into one graph and replayed.  Materials, BSDFs and image
accumulation stay with the caller.

Buffers are torch tensors on the accel's device: ray / hit records are uint8 tensors of 32 bytes per slot (RTRay / RTHitResult, view them
with RAY_DT / HIT_DT), path ids and counts are int32 tensors holding u32 values.
"""
import math

import numpy as np

from ._capi import RaycoreError

RC_INVALID_ID = 0xFFFFFFFF


def lookat_camera(eye, target, width, height, fov_deg=45.0, up=(0.0, 1.0, 0.0)):
    """Camera basis for primary_rays_lookat_device: dict(pos, right, up, forward, half_width, half_height), float32."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    half_h = np.tan(np.radians(fov_deg) / 2)
    return {"pos": eye.astype(np.float32), "right": r.astype(np.float32), "up": u.astype(np.float32), "forward": f.astype(np.float32),
            "half_width": float(np.float32(half_h * width / height)), "half_height": float(np.float32(half_h))}


def _stream(stream):
    import torch
    return stream if stream is not None else torch.cuda.current_stream()


def check_ao_arguments(n, ao_samples, ao_distance):
    """(ao_samples, ao_distance) as (int, float) for a frame of n paths, or ValueError: what rc_ambient_occlusion_device would refuse, said
    before a device is touched."""
    if isinstance(ao_samples, bool) or ao_samples != int(ao_samples) or not 0 <= int(ao_samples) < 65536:
        raise ValueError("ao_samples must be an integer in [0, 65536)")
    if not float(ao_distance) > 0.0:  # (NaN included; inf is legal)
        raise ValueError("ao_distance must be > 0 (inf: unbounded)")
    if int(n) * int(ao_samples) >= 2 ** 32:
        raise ValueError("width * height * samples * ao_samples must be below 2^32")
    return int(ao_samples), float(ao_distance)


def check_gather_arguments(n, samples, distance, miss_value):
    """(samples, distance, miss_value) as (int, float, int) for a frame of n paths, or ValueError: what rc_final_gather_device would
    refuse -- and a miss_value that is no u32 --, said before a device is touched."""
    if isinstance(samples, bool) or samples != int(samples) or not 0 <= int(samples) < 65536:
        raise ValueError("samples must be an integer in [0, 65536)")
    if not float(distance) > 0.0:  # (NaN included; inf is legal)
        raise ValueError("distance must be > 0 (inf: unbounded)")
    if isinstance(miss_value, bool) or miss_value != int(miss_value) or not 0 <= int(miss_value) < 2 ** 32:
        raise ValueError("miss_value must be an integer in [0, 2^32)")
    if int(n) * int(samples) >= 2 ** 32:
        raise ValueError("the number of hits times samples must be below 2^32")
    return int(samples), float(distance), int(miss_value)


class WavefrontPaths:
    """Owns the device buffers of a `depth`-deep path frame of width*height*samples paths on `accel` (a synced TLAS) and enqueues it.

    Per depth b (0-based): rays[b] / hits[b] (the closest-hit stage), shadow_rays[b] / shadow_hits[b] (any_hit toward `light`) and
    path_ids[b] (the path each slot of rays[b] continues; path_ids[0] is the primary ray index, dead slots hold RC_INVALID_ID).
    compact=True gathers the hits into a live-first queue (compact_hits_device) before each bounce, so the live slots come first and the
    dead tail is traced as rays that miss; compact=False keeps slot i on path i.  A path's bounce directions depend only on
    (seed, path id, depth), so both modes produce the same (path id -> hit) records.

    dynamic: a list of (handle, transforms tensor) pairs -- float32 (m, 12) or (m, 3, 4) on the accel's device.  Every frame then starts
    with update_transforms_device for each pair and one refit_device_async on the frame's stream, before the primary rays: the frame
    shows whatever the tensors hold when it runs, also when it is a replay of the captured graph.

    rebuild=True (needs `dynamic`): the head of every frame calls rebuild_device_async instead of refit_device_async, so every frame
    traces the tree a fresh sync would build from the tensors' transforms.  A caller who wants a rebuild only every K frames keeps the
    default and calls accel.rebuild_device_async(stream) eagerly between replays of the captured refit frame: the rebuild works in place,
    so the captured graph stays valid and refits the new topology from then on.

    rebuild="auto" (needs `dynamic`): the head of every frame calls refit_or_rebuild_device_async(self.rebuild_ratio) -- a refit, and a
    rebuild only on the frames whose refitted tree costs more than rebuild_ratio x what the tree cost when it was last built, decided on
    the device, so one captured frame takes either path from replay to replay.  The constructor makes the eager arming call (a refit and
    a rebuild of the accel's current transforms on the current stream, waited for), so capture() works at once; accel.tlas_quality()
    reads the decisions back.  The ratio is the attribute rebuild_ratio, 1.5 unless the caller sets it before run() / capture() (a
    captured frame keeps the ratio it was captured with; the constructor's parameter list is pinned by tests/test_soft_shadow_api.py, so
    it is not a keyword).  1.5 is a judgement: no measurement stands behind it.  profiles/tlas_auto_rebuild.json (tools/probes/tlas_rebuild_probe.py)
    has one curve of cost and trace time against the fraction of instances exchanged, on C3, from which a later change can choose.

    deform: a list of (handle, soup tensor) pairs -- float32 (n, 9) or (n, 3, 3) on the accel's device.  Every frame then starts with
    update_geometry_device_async for each pair, before the `dynamic` transform updates and the refit (or rebuild) that ends the head of
    the frame; `deform` without `dynamic` still ends it with a refit.  A soup must keep its number of non-degenerate faces.

    lights + fused_shadows=True: several point lights tested in one launch per depth.  `lights` is a float32 (L, 3) tensor on the accel's
    device (or an array, uploaded once into self.lights); each depth then runs one shadow_visibility_device into visible[b], a uint8 tensor
    of n * L bytes (byte i * L + l: slot i of hits[b] is lit by light l), and shadow_rays[b] / shadow_hits[b] do not exist (empty lists).
    The lights are read when the frame runs: in-place edits of the tensor show up in the next run() or replay().  `light` is not used then.

    shadow_samples > 1 (needs fused_shadows=True and light_radii): soft shadows.  `light_radii` is a float32 (L,) tensor on the accel's
    device (or an array, uploaded once into self.light_radii), read when the frame runs like `lights`.  Each depth b then zeroes
    shadow_counts[b] (an int32 tensor holding n * L u32 counts) on the frame's stream and runs one soft_shadow_visibility_device with
    depth=b, d_path_in=path_ids[b] and the frame's seed: count i * L + l is the number of the shadow_samples samples of light l that slot i
    of hits[b] sees, a path's samples do not depend on compaction, and visible[b] is not produced (an empty list).  light_radii with
    shadow_samples == 1 is refused: one sample is the hard shadow and would ignore the radii.

    Ambient occlusion: with_ambient_occlusion(ao_samples, ao_distance=inf) after the constructor (which leaves ao_samples = 0; like
    rebuild_ratio it is not a constructor keyword, for the same reason).  With ao_samples > 0 each depth b, after its shadow stage,
    zeroes ao_counts[b] (an int32 tensor holding n u32 counts) on the frame's stream and runs one ambient_occlusion_device with
    max_dist=ao_distance, depth=b, d_path_in=path_ids[b] and the frame's seed and bias: count i is the number of the ao_samples
    cosine-weighted hemisphere samples of slot i of hits[b] that reach ao_distance unoccluded, and a path's samples do not depend on
    compaction.  With ao_samples == 0 the frame is what it was: no launch, no buffer, the same traced_rays().

    Final gather: with_final_gather(x, samples, distance=inf, miss_value=0) after the constructor, like the ambient-occlusion switch.  x is
    an int32 tensor on the accel's device holding one u32 per primitive (indexed by metadata - 1: a radiosity iterate, say), held by
    reference and read by every frame when its kernels run.  With samples > 0 each depth b, after the ambient-occlusion stage, zeroes
    gather_sums[b] (int64, n) and gather_open[b] (int32, n) on the frame's stream and runs one final_gather_device with
    max_dist=distance, depth=b, d_path_in=path_ids[b] and the frame's seed and bias: sum i is x summed over what the `samples` hemisphere
    samples of slot i of hits[b] hit first (miss_value for one that escapes), open i the samples that escape -- the ambient-occlusion
    stage's rays, so with equal samples and distance gather_open[b] equals ao_counts[b].  With samples == 0 the frame is what it was.

    Placed final gather: with_placed_final_gather(x, samples, distance=inf, miss_value=0), the same stage with x an int32 tensor holding one
    u32 per PLACED primitive (indexed by q = base[instance] + l: placed_radiosity's result, say) and one placed_final_gather_device per
    depth.  A frame has ONE gather stage, metadata or placed: both switches write the gather_* fields and the flag gather_placed, and the
    last one called wins."""

    def __init__(self, accel, width, height, samples, depth, camera, light=None, seed=0, bias=1e-3, compact=True, dynamic=None, rebuild=False,
                 deform=None, lights=None, fused_shadows=False, shadow_samples=1, light_radii=None):
        if depth < 1:
            raise ValueError("depth must be at least 1")
        if isinstance(rebuild, (str, tuple)) and rebuild != "auto":
            raise ValueError('rebuild must be False, True or "auto"')
        if rebuild and not dynamic:
            raise ValueError("rebuild=True needs dynamic: the rebuild follows the transform updates at the head of the frame")
        self.fused_shadows = bool(fused_shadows)
        if lights is not None and not self.fused_shadows:
            raise ValueError("lights= needs fused_shadows=True: the composed stages trace one `light`")
        if self.fused_shadows and lights is None:
            raise ValueError("fused_shadows=True needs lights=: a float32 (L, 3) tensor or array of point-light positions")
        if not self.fused_shadows and light is None:
            raise ValueError("light is required (or lights= with fused_shadows=True)")
        if self.fused_shadows:
            shape = tuple(lights.shape) if hasattr(lights, "shape") else np.asarray(lights).shape
            if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
                raise ValueError("lights must have shape (L, 3) with L >= 1")
            if int(width) * int(height) * int(samples) * shape[0] >= 2 ** 32:
                raise ValueError("width * height * samples * L must be below 2^32")
        self.shadow_samples = int(shadow_samples)
        if not 1 <= self.shadow_samples < 65536:
            raise ValueError("shadow_samples must be in [1, 65536)")
        if self.shadow_samples == 1 and light_radii is not None:
            raise ValueError("light_radii needs shadow_samples > 1: one sample per light is the hard shadow, which has no radius")
        if self.shadow_samples > 1:
            if not self.fused_shadows:
                raise ValueError("shadow_samples > 1 needs fused_shadows=True: soft shadows are one launch over hits x lights x samples")
            if light_radii is None:
                raise ValueError("shadow_samples > 1 needs light_radii=: a float32 (L,) tensor or array of area-light radii")
            if shape[0] >= 65536:
                raise ValueError("shadow_samples > 1 takes fewer than 65536 lights")
            rshape = tuple(light_radii.shape) if hasattr(light_radii, "shape") else np.asarray(light_radii).shape
            if rshape != (shape[0],):
                raise ValueError("light_radii must have shape (L,), one radius per light")
            if int(width) * int(height) * int(samples) * shape[0] * self.shadow_samples >= 2 ** 32:
                raise ValueError("width * height * samples * L * shadow_samples must be below 2^32")
        import torch
        self.accel, self.width, self.height, self.samples, self.depth = accel, int(width), int(height), int(samples), int(depth)
        self.n = self.width * self.height * self.samples
        if self.n == 0 or self.n >= 2 ** 31:
            raise ValueError("width * height * samples must be in [1, 2^31)")
        self.camera = {k: (np.asarray(v, np.float32) if k in ("pos", "right", "up", "forward") else float(v)) for k, v in camera.items()}
        self.light = None if light is None else np.ascontiguousarray(light, dtype=np.float32)
        self.seed, self.bias, self.compact = int(seed), float(bias), bool(compact)
        self.dynamic = list(dynamic) if dynamic else []
        self.rebuild = "auto" if rebuild == "auto" else bool(rebuild)
        self.rebuild_ratio = 1.5
        self.ao_samples, self.ao_distance, self.ao_counts = 0, math.inf, []
        self.gather_samples, self.gather_distance, self.gather_miss, self.gather_x, self.gather_sums, self.gather_open = 0, math.inf, 0, None, [], []
        self.gather_placed = False  # which call the gather stage makes: final_gather_device, or placed_final_gather_device (with_placed_final_gather)
        self.deform = list(deform) if deform else []
        dev = torch.device("cuda", accel.device)
        rec = lambda: torch.zeros(self.n * 32, dtype=torch.uint8, device=dev)  # noqa: E731
        self.rays = [rec() for _ in range(depth)]
        self.hits = [rec() for _ in range(depth)]
        self.lights, self.n_lights, self.visible = None, 0, []
        if self.fused_shadows:
            if isinstance(lights, torch.Tensor):
                if lights.dtype != torch.float32 or lights.device != dev or not lights.is_contiguous():
                    raise ValueError("lights must be a contiguous float32 tensor on the accel's device")
                self.lights = lights
            else:
                self.lights = torch.from_numpy(np.ascontiguousarray(lights, dtype=np.float32)).to(dev)
            self.n_lights = int(self.lights.shape[0])
            if self.shadow_samples == 1:
                self.visible = [torch.zeros(self.n * self.n_lights, dtype=torch.uint8, device=dev) for _ in range(depth)]
        self.light_radii, self.shadow_counts = None, []
        if self.shadow_samples > 1:
            if isinstance(light_radii, torch.Tensor):
                if light_radii.dtype != torch.float32 or light_radii.device != dev or not light_radii.is_contiguous():
                    raise ValueError("light_radii must be a contiguous float32 tensor on the accel's device")
                self.light_radii = light_radii
            else:
                self.light_radii = torch.from_numpy(np.ascontiguousarray(light_radii, dtype=np.float32)).to(dev)
            self.shadow_counts = [torch.zeros(self.n * self.n_lights, dtype=torch.int32, device=dev) for _ in range(depth)]
        self.shadow_rays = [] if self.fused_shadows else [rec() for _ in range(depth)]
        self.shadow_hits = [] if self.fused_shadows else [rec() for _ in range(depth)]
        self.path_ids = [torch.arange(self.n, dtype=torch.int32, device=dev)] + [
            torch.full((self.n,), -1, dtype=torch.int32, device=dev) for _ in range(depth - 1)]
        self.indices = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        # the buffers are initialised on the allocating stream; a frame may run on any other: wait for them once, here
        torch.cuda.current_stream(dev).synchronize()
        self._streams = set()
        self.graph = None
        self._graph_stream = None
        if self.rebuild == "auto" and not accel.tlas_quality()["armed"]:  # the arming call is eager by contract: here, so that capture() works
            accel.refit_or_rebuild_device_async(self.rebuild_ratio, stream=torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.current_stream(dev).synchronize()

    def with_ambient_occlusion(self, ao_samples, ao_distance=math.inf):
        """Switch the frame's ambient-occlusion stage on (ao_samples > 0) or off (0), before the next run() or capture(); returns self.
        ValueError for ao_samples outside [0, 65536), an ao_distance that is not > 0, or width*height*samples*ao_samples >= 2^32 -- all
        before a tensor is made.  A captured frame keeps the stage it was captured with, so it is refused here."""
        ao_samples, ao_distance = check_ao_arguments(self.n, ao_samples, ao_distance)
        if self._graph_stream is not None:
            raise RaycoreError(1, "WavefrontPaths.with_ambient_occlusion: this frame is already captured")
        import torch
        dev = torch.device("cuda", self.accel.device)
        counts = [torch.zeros(self.n, dtype=torch.int32, device=dev) for _ in range(self.depth)] if ao_samples else []
        torch.cuda.current_stream(dev).synchronize()  # (as in the constructor: a frame may run on another stream than the allocating one)
        self.ao_samples, self.ao_distance, self.ao_counts = ao_samples, ao_distance, counts
        self._streams = set()  # the new buffers are recorded on a stream at its next run()
        return self

    def with_final_gather(self, x, samples, distance=math.inf, miss_value=0):
        """Switch the frame's final-gather stage on (samples > 0) or off (0), before the next run() or capture(); returns self.  x: an
        int32 tensor of n_primitives words on the accel's device (u32 values, indexed by metadata - 1), kept by reference and read each
        frame.  ValueError for samples outside [0, 65536), a distance that is not > 0, a miss_value that is no u32,
        width*height*samples*samples >= 2^32 or an x of another kind -- all before a tensor is made.  A captured frame keeps the stage it
        was captured with, so it is refused here."""
        return self._set_gather(False, x, samples, distance, miss_value)

    def with_placed_final_gather(self, x, samples, distance=math.inf, miss_value=0):
        """with_final_gather for a field per PLACED primitive: x is an int32 tensor of placed_primitive_count words on the accel's device
        (u32 values, indexed by placed primitive q = base[instance] + l), and each depth runs one placed_final_gather_device instead.  The
        same checks, buffers (gather_sums, gather_open) and refusal of a captured frame.  The frame has one gather stage: this call
        replaces a with_final_gather stage and the other way round."""
        return self._set_gather(True, x, samples, distance, miss_value)

    def _set_gather(self, placed, x, samples, distance, miss_value):
        """The body of the two gather switches: `placed` picks the index space of x and the call run() makes."""
        samples, distance, miss_value = check_gather_arguments(self.n, samples, distance, miss_value)
        name = "with_placed_final_gather" if placed else "with_final_gather"
        if self._graph_stream is not None:
            raise RaycoreError(1, f"WavefrontPaths.{name}: this frame is already captured")
        import torch
        dev = torch.device("cuda", self.accel.device)
        if samples:
            if not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.dim() != 1 or x.device != dev or not x.is_contiguous():
                raise ValueError("x must be a contiguous one-dimensional int32 tensor on the accel's device")
            if placed:
                count = int(self.accel.placed_primitive_bases()[-1])
                if x.numel() != count:
                    raise ValueError(f"x must hold one value per placed primitive: {x.numel()} values for {count} placed primitives")
            elif x.numel() != self.accel.n_primitives():
                raise ValueError(f"x must hold one value per primitive: {x.numel()} values for {self.accel.n_primitives()} primitives")
        sums = [torch.zeros(self.n, dtype=torch.int64, device=dev) for _ in range(self.depth)] if samples else []
        opened = [torch.zeros(self.n, dtype=torch.int32, device=dev) for _ in range(self.depth)] if samples else []
        torch.cuda.current_stream(dev).synchronize()  # (as in the constructor: a frame may run on another stream than the allocating one)
        self.gather_samples, self.gather_distance, self.gather_miss = samples, distance, miss_value
        self.gather_x, self.gather_sums, self.gather_open = (x if samples else None), sums, opened
        self.gather_placed = bool(placed) and samples > 0
        self._streams = set()  # the new buffers are recorded on a stream at its next run()
        return self

    def buffers(self):
        fused = self.visible + [self.lights] if self.fused_shadows else []
        if self.shadow_samples > 1:
            fused = fused + self.shadow_counts + [self.light_radii]
        return self.rays + self.hits + self.shadow_rays + self.shadow_hits + fused + self.ao_counts + self.gather_sums + self.gather_open + ([self.gather_x] if self.gather_samples else []) + self.path_ids + [self.indices, self.count] + [t for _, t in self.dynamic] + [t for _, t in self.deform]

    def run(self, stream=None):
        """Enqueue one frame on `stream` (a torch.cuda.Stream; None = the current stream).  No host synchronisation.  The first frame on
        a stream must run eagerly, before any capture on it."""
        import torch
        s = _stream(stream)
        st = s.cuda_stream
        if st not in self._streams:  # the caching allocator must not hand the buffers out again while this stream may still use them
            for buf in self.buffers():
                buf.record_stream(s)
            self._streams.add(st)
        a, c, n = self.accel, self.camera, self.n
        for handle, soup in self.deform:
            a.update_geometry_device_async(handle, soup, stream=st)
        if self.dynamic or self.deform:
            for handle, xf in self.dynamic:
                a.update_transforms_device(handle, xf, stream=st)
            if self.rebuild == "auto":
                a.refit_or_rebuild_device_async(self.rebuild_ratio, stream=st)
            elif self.rebuild:
                a.rebuild_device_async(stream=st)
            else:
                a.refit_device_async(stream=st)
        a.primary_rays_lookat_device(c["pos"], c["right"], c["up"], c["forward"], c["half_width"], c["half_height"], self.width, self.height,
                                     self.rays[0].data_ptr(), samples=self.samples, seed=self.seed, jitter=True, stream=st)
        a.trace_device(self.rays[0].data_ptr(), self.hits[0].data_ptr(), n, stream=st)
        for b in range(self.depth):
            if self.shadow_samples > 1:
                with torch.cuda.stream(s):  # the call accumulates: zero on the frame's stream, whichever stream is current
                    self.shadow_counts[b].zero_()
                a.soft_shadow_visibility_device(self.rays[b].data_ptr(), self.hits[b].data_ptr(), n, self.lights.data_ptr(), self.light_radii.data_ptr(),
                                                self.n_lights, self.shadow_samples, self.shadow_counts[b].data_ptr(), seed=self.seed, depth=b,
                                                bias=self.bias, d_path_in=self.path_ids[b].data_ptr(), stream=st)
            elif self.fused_shadows:
                a.shadow_visibility_device(self.rays[b].data_ptr(), self.hits[b].data_ptr(), n, self.lights.data_ptr(), self.n_lights,
                                           self.visible[b].data_ptr(), bias=self.bias, stream=st)
            else:
                a.shadow_rays_device(self.rays[b].data_ptr(), self.hits[b].data_ptr(), n, self.light, self.shadow_rays[b].data_ptr(),
                                     bias=self.bias, stream=st)
                a.trace_device(self.shadow_rays[b].data_ptr(), self.shadow_hits[b].data_ptr(), n, mode="any", stream=st)
            if self.ao_samples > 0:
                with torch.cuda.stream(s):  # the call accumulates: zero on the frame's stream, whichever stream is current
                    self.ao_counts[b].zero_()
                a.ambient_occlusion_device(self.rays[b].data_ptr(), self.hits[b].data_ptr(), n, self.ao_samples, self.ao_counts[b].data_ptr(),
                                           max_dist=self.ao_distance, seed=self.seed, depth=b, bias=self.bias,
                                           d_path_in=self.path_ids[b].data_ptr(), stream=st)
            if self.gather_samples > 0:
                with torch.cuda.stream(s):  # the call accumulates: zero on the frame's stream, whichever stream is current
                    self.gather_sums[b].zero_()
                    self.gather_open[b].zero_()
                gather = a.placed_final_gather_device if self.gather_placed else a.final_gather_device
                gather(self.rays[b].data_ptr(), self.hits[b].data_ptr(), n, self.gather_samples, self.gather_x.data_ptr(),
                       self.gather_sums[b].data_ptr(), self.gather_open[b].data_ptr(), miss_value=self.gather_miss,
                       max_dist=self.gather_distance, seed=self.seed, depth=b, bias=self.bias,
                       d_path_in=self.path_ids[b].data_ptr(), stream=st)
            if b + 1 >= self.depth:
                break
            src = cnt = None
            if self.compact:
                a.compact_hits_device(self.hits[b].data_ptr(), n, self.indices.data_ptr(), self.count.data_ptr(), stream=st)
                src, cnt = self.indices.data_ptr(), self.count.data_ptr()
            a.bounce_rays_device(self.rays[b].data_ptr(), self.hits[b].data_ptr(), n, self.rays[b + 1].data_ptr(), seed=self.seed,
                                 bounce=b, bias=self.bias, d_src=src, d_src_count=cnt, d_path_in=self.path_ids[b].data_ptr(),
                                 d_path_out=self.path_ids[b + 1].data_ptr(), stream=st)
            a.trace_device(self.rays[b + 1].data_ptr(), self.hits[b + 1].data_ptr(), n, stream=st)

    def capture(self, stream):
        """Record one frame into a torch.cuda.CUDAGraph on `stream`, which must have run the frame eagerly before (the trace needs its
        stack spill area, the compaction its scratch: include/raycore_mi355x.h, "hipGraph capture").  The graph holds 2 * depth of the
        scene's 16 captured launches until the caller destroys it and hands them back (accel.set_option("release_captures", 1))."""
        import torch
        if self._graph_stream is not None:
            raise RaycoreError(1, "WavefrontPaths.capture: this frame is already captured")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            self.run(stream)
        self.graph, self._graph_stream = g, stream
        return g

    def replay(self):
        """Replay the captured frame (asynchronous, like run)."""
        if self.graph is None:
            raise RaycoreError(1, "WavefrontPaths.replay: capture() a frame first")
        self.graph.replay()

    def traced_rays(self):
        """Ray slots one frame traces: per depth one closest-hit pass (primary or bounce) and one any-hit pass (shadow) over every slot,
        dead ones included -- with fused_shadows one any-hit item per slot and light, with shadow_samples > 1 per slot, light and sample;
        with ao_samples > 0 one more any-hit item per slot and sample, with the final gather one more closest-hit item per slot and sample."""
        return (self.n * (1 + (self.n_lights * self.shadow_samples if self.fused_shadows else 1)) * self.depth + self.n * self.ao_samples * self.depth
                + self.n * self.gather_samples * self.depth)


def c4_bounce_rays_device(accel, d_rays, d_hits, n_primary, n_rays, d_out, seed=0xC4, stream=None):
    """C4's incoherent diffuse bounce rays made on the device: the n_primary primary hits are compacted and reused round robin
    (rc_bounce_rays_device with wrap=1) to fill n_rays output slots at d_out, origin = hit point + 1e-3 * normal, path id = the primary
    ray's index.  `stream`: a torch.cuda.Stream (None = the current one).  Returns the (indices, count) tensors the call reads on the
    device; they are also recorded on the stream, so dropping them is safe."""
    import torch
    s = _stream(stream)
    dev = torch.device("cuda", accel.device)
    indices = torch.empty(max(int(n_primary), 1), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    if s != torch.cuda.current_stream(dev):
        indices.record_stream(s)
        count.record_stream(s)
    accel.compact_hits_device(d_hits, int(n_primary), indices.data_ptr(), count.data_ptr(), stream=s.cuda_stream)
    accel.bounce_rays_device(d_rays, d_hits, int(n_rays), d_out, seed=seed, bounce=0, bias=1e-3, d_src=indices.data_ptr(),
                             d_src_count=count.data_ptr(), wrap=True, stream=s.cuda_stream)
    return indices, count

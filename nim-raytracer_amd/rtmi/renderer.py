"""Renderer API over librtmi.so, mirroring src/renderer/renderer.nim.

    initRenderer(device)                         renderer.nim:214-215
    renderLine(scene, opts, fb, y, step, maxStep) -> Stats
                                                 renderer.nim:162-211
plus the whole-frame and multi-GPU forms that replace the scanline worker
pool (src/raytracer.nim:25-109, src/concurrency/workerpool.nim) with one GPU
dispatch. `scene` is the reference's Scene (renderLine caches its device copy,
as the Nim binding in INTEGRATION.md does) or a DeviceScene: the Scene flattened and
uploaded once (BVH built) — the Nim shim in INTEGRATION.md does the same.
"""
import contextlib
import ctypes as C
import threading
from types import SimpleNamespace

import numpy as np

from . import abi, glm
from ._lib import RtmiError, check, lib
from .scene import Options, Scene, Stats, flatten, flatten_lights, flatten_objects


def initRenderer(device=0):
    """Bind this thread to GPU `device` (must be gfx950)."""
    check(lib().rt_init(int(device)))


def device_count():
    return int(lib().rt_device_count())


class DeviceScene:
    """A Scene resident in HBM on one GPU (objects, lights, BVH, triangles)."""

    def __init__(self, scene: Scene, device=0, bvh_builder=abi.RT_BVH_SAH):
        """bvh_builder: abi.RT_BVH_SAH (host binned SAH, default) or
        abi.RT_BVH_PLOC (built on the GPU); images and Stats are the same."""
        initRenderer(device)
        self.device = device
        self.scene = scene
        flat = flatten(scene)
        flat.desc.bvh_builder = int(bvh_builder)
        h = C.c_void_p()
        check(lib().rt_scene_create(C.byref(flat.desc), C.byref(h)))
        self.h = h
        self._mesh_ids = [id(g) for g in flat._meshes]  # rt_scene_desc.meshes order (set_mesh_vertices)
        self._kinds = _object_kinds(flat._objs, len(scene.objects))  # what set_objects keeps

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().rt_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = abi.rt_scene_info()
        check(lib().rt_scene_get_info(self.h, C.byref(i)))
        return i.as_dict()

    def set_camera(self, cameraToWorld=None, fov=None):
        """Scene.cameraToWorld / Scene.fov for the next render calls
        (renderLine re-reads them every call, renderer.nim:135-136,150-153);
        None: this DeviceScene's Scene's current values."""
        m = self.scene.cameraToWorld if cameraToWorld is None else cameraToWorld
        f = self.scene.fov if fov is None else fov
        arr = (C.c_double * 16)(*[float(x) for x in glm.flat(m)])
        check(lib().rt_scene_set_camera(self.h, arr, float(f)))

    def set_lights(self, lights=None):
        """Scene.lights for the next calls (rt_scene_set_lights): any number
        and mix of DistantLight / PointLight; None: this DeviceScene's
        Scene's current lights. The geometry, BVH and camera stay; the
        scene then renders exactly as one created with these lights."""
        ls = list(self.scene.lights if lights is None else lights)
        check(lib().rt_scene_set_lights(self.h, flatten_lights(ls), len(ls)))

    def set_objects(self, objects=None):
        """Scene.objects' placement and materials for the next calls
        (rt_scene_set_objects): every object's objectToWorld / worldToObject,
        sphere radius, box bounds, albedo and reflection; None: this
        DeviceScene's Scene's current objects. The list must hold the same
        number of objects of the same kinds (and, for meshes, the same
        TriangleMesh) as at create: TypeError / ValueError otherwise, before
        the device is touched. Meshes, BVH, lights and camera stay; the scene
        then answers exactly as one created with these objects."""
        objs = list(self.scene.objects if objects is None else objects)
        arr = _checked_objects(objs, self._mesh_ids, self._kinds)
        check(lib().rt_scene_set_objects(self.h, arr, len(objs)))

    def mesh_index(self, mesh):
        """The rt_scene_desc.meshes index of `mesh`: an index, or one of the
        TriangleMesh objects this DeviceScene was created from."""
        if isinstance(mesh, (int, np.integer)):
            return int(mesh)
        try:
            return self._mesh_ids.index(id(mesh))
        except ValueError:
            raise ValueError("mesh is not one of this DeviceScene's TriangleMesh objects") from None

    def set_mesh_vertices(self, mesh, vertices, normals=None, stream=None):
        """New vertex positions for one mesh (rt_scene_set_mesh_vertices):
        `mesh` is an index or the scene's TriangleMesh, vertices (N, 3)
        float64 with the N the mesh was created with, normals (F, 3) or None
        (calcNormals, as at create). numpy arrays take the host form; float64
        CUDA tensors the device form, read behind `stream` (None: torch's
        current stream). Faces, BVH topology, camera, lights and the other
        meshes stay; the scene then answers exactly as one created with
        these vertices."""
        m = self.mesh_index(mesh)
        if _is_host(vertices):
            v = _host_f64(vertices, (-1, 3))
            n = None if normals is None else _host_f64(normals, (-1, 3))
            check(lib().rt_scene_set_mesh_vertices(self.h, m, _dptr(v), v.shape[0], _dptr(n)))
            return
        nv = _dev_f64(vertices, None, 3)
        if normals is not None:
            if _is_host(normals):
                raise ValueError("vertices and normals must both be host arrays or both device tensors")
            _dev_f64(normals, None, 3)
        check(lib().rt_scene_set_mesh_vertices_device(
            self.h, m, C.c_void_p(vertices.data_ptr()), nv,
            C.c_void_p(normals.data_ptr()) if normals is not None else None, _stream(stream)))

    # -- host framebuffer (the pool-compatible path) ----------------------
    def render_lines(self, opts: Options, fb, y0, y1, step=1, maxStep=1) -> Stats:
        """renderLine for every y in countup(y0, y1-1, step); fb is a
        C-contiguous float32 array of shape (h, w, 3) (framebuf.nim layout)."""
        if not (isinstance(fb, np.ndarray) and fb.dtype == np.float32 and fb.flags.c_contiguous
                and fb.shape == (opts.height, opts.width, 3)):
            raise ValueError("fb must be a C-contiguous float32 array of shape (height, width, 3)")
        o = opts.to_c()
        st = abi.rt_stats()
        check(lib().rt_render_lines(self.h, C.byref(o), fb.ctypes.data_as(C.POINTER(C.c_float)),
                                    opts.width, opts.height, int(y0), int(y1), int(step),
                                    int(maxStep), C.byref(st)))
        return Stats.from_c(st)

    # -- device framebuffer (the fast path) --------------------------------
    def render_device(self, opts: Options, d_fb, y0=0, y1=None, step=1, maxStep=1, stream=None,
                      stats=True):
        """Render rows into a device buffer (int pointer or torch tensor of
        height*width*3 float32). With stats=False nothing synchronises."""
        ptr = _ptr(d_fb, opts.width * opts.height * 3)
        o = opts.to_c()
        st = abi.rt_stats()
        check(lib().rt_render_lines_device(self.h, C.byref(o), C.c_void_p(ptr), int(y0),
                                           int(opts.height if y1 is None else y1), int(step),
                                           int(maxStep), _stream(stream),
                                           C.byref(st) if stats else None))
        return Stats.from_c(st) if stats else None

    def render_bands_device(self, opts: Options, d_bands, band_h, rank, world, stream=None,
                            stats=True):
        rows = band_rows(opts.height, band_h, world)
        ptr = _ptr(d_bands, rows * opts.width * 3)
        o = opts.to_c()
        st = abi.rt_stats()
        check(lib().rt_render_bands_device(self.h, C.byref(o), C.c_void_p(ptr), int(band_h), int(rank),
                                           int(world), _stream(stream), C.byref(st) if stats else None))
        return Stats.from_c(st) if stats else None

    # -- ray queries (rt_trace_rays* / rt_pick_pixels*) ----------------------
    def trace_rays(self, orig, dir, t_near=None, any_hit=False, sort=False, normals=False, stats=False,
                   stream=None):
        """trace (renderer.nim:47-67) for n rays: orig and dir are (n, 3)
        float64 — numpy arrays (the host form) or CUDA torch tensors (the
        device form, enqueued on `stream`; it waits only with stats=True) —
        dir as given, not normalised; t_near (n,) or None for +inf. Returns
        (t, obj, face[, normals][, Stats]) as arrays of the same kind: t is
        the ray's t_near and obj / face are -1 on a miss; with any_hit only
        obj >= 0 / obj == -1 is meaningful; sort traces the rays in a
        coherence order (the same answers); normals: shade's hitNormal per
        hit, (0, 0, 0) on a miss. The device form's t / obj / face are views
        of one (n, 2) float64 tensor."""
        flags = (abi.RT_QUERY_ANY_HIT if any_hit else 0) | (abi.RT_QUERY_SORT if sort else 0)
        if _is_host(orig):
            o, d = _host_f64(orig, (-1, 3)), _host_f64(dir, (-1, 3))
            n = o.shape[0]
            if d.shape[0] != n:
                raise ValueError("orig and dir must hold the same number of rays")
            tn = None if t_near is None else _host_f64(t_near, (n,))
            return self._query_host(_HITS64, n, normals, stats, lambda hits, nrm, st: lib().rt_trace_rays(
                self.h, n, _dptr(o), _dptr(d), _dptr(tn), flags, hits, nrm, st))
        n = _dev_f64(orig, None, 3)
        _dev_f64(dir, n, 3)
        if t_near is not None:
            _dev_f64(t_near, n, 1)
        return self._query_device(_HITS64, orig, n, normals, stats, lambda hits, nrm, st: lib().rt_trace_rays_device(
            self.h, n, C.c_void_p(orig.data_ptr()), C.c_void_p(dir.data_ptr()),
            C.c_void_p(t_near.data_ptr()) if t_near is not None else None, flags, hits, nrm, _stream(stream), st))

    def pick(self, opts: Options, xy, any_hit=False, sort=False, normals=False, stats=False, stream=None):
        """What is under image position xy[i] = (x, y): castPrimaryRay
        (renderer.nim:31-44) through the scene's current camera for an
        opts.width x opts.height image (opts.precision must be fp64), then
        trace with t_near = +inf. Integer (x, y) is the akNone sample of that
        pixel; fractional and out-of-image positions are legal. xy is (n, 2)
        float64, numpy or CUDA torch; returns as trace_rays does, the Stats'
        numPrimaryRays counting the rays that are not degenerate."""
        flags = (abi.RT_QUERY_ANY_HIT if any_hit else 0) | (abi.RT_QUERY_SORT if sort else 0)
        o = opts.to_c()
        if _is_host(xy):
            p = _host_f64(xy, (-1, 2))
            n = p.shape[0]
            return self._query_host(_HITS64, n, normals, stats, lambda hits, nrm, st: lib().rt_pick_pixels(
                self.h, C.byref(o), n, _dptr(p), flags, hits, nrm, st))
        n = _dev_f64(xy, None, 2)
        return self._query_device(_HITS64, xy, n, normals, stats, lambda hits, nrm, st: lib().rt_pick_pixels_device(
            self.h, C.byref(o), n, C.c_void_p(xy.data_ptr()), flags, hits, nrm, _stream(stream), st))

    # -- radiance queries (rt_shade_rays*) -----------------------------------
    def shade_rays(self, opts: Options, orig, dir, group=1, sort=False, f32=False, stats=False, stream=None):
        """shade(ray, trace(ray)) (renderer.nim:47-127) for n caller-supplied
        rays — the reference's colour along each, whatever camera formed it;
        the scene's own camera is not read. orig and dir are (n, 3) float64,
        numpy arrays (the host form) or CUDA torch tensors (the device form,
        enqueued on `stream`; it waits only with stats=True); dir as given,
        not normalised. Of opts only bias, maxRayDepth and precision (fp64)
        are read. group=1: one colour per ray; group=g: calcPixel's mean of
        each run of g rays, summed in index order. Returns rgb as an
        (n / group, 3) array of the same kind, float64 or (f32=True) float32
        as Framebuf stores it, then the Stats when asked. A degenerate ray
        (a non-finite component, a zero direction) is (0, 0, 0) and counts
        nowhere; sort traces the rays in a coherence order (the same answers)."""
        flags = abi.RT_QUERY_SORT if sort else 0
        group = int(group)
        o = opts.to_c()
        st = abi.rt_stats()
        pst = C.byref(st) if stats else None
        if _is_host(orig):
            og, d = _host_f64(orig, (-1, 3)), _host_f64(dir, (-1, 3))
            n = og.shape[0]
            if d.shape[0] != n:
                raise ValueError("orig and dir must hold the same number of rays")
            ng = n // group if group >= 1 and n % group == 0 else 0  # (the library reports a bad group)
            rgb = np.zeros((ng, 3), dtype=np.float32 if f32 else np.float64)
            check(lib().rt_shade_rays(self.h, C.byref(o), n, _dptr(og), _dptr(d), group, flags,
                                      None if f32 else _dptr(rgb),
                                      rgb.ctypes.data_as(C.POINTER(C.c_float)) if f32 else None, pst))
            return (rgb, Stats.from_c(st)) if stats else rgb
        import torch
        n = _dev_f64(orig, None, 3)
        _dev_f64(dir, n, 3)
        ng = n // group if group >= 1 and n % group == 0 else 0
        rgb = torch.empty((ng, 3), dtype=torch.float32 if f32 else torch.float64, device=orig.device)
        p = C.c_void_p(rgb.data_ptr())
        check(lib().rt_shade_rays_device(self.h, C.byref(o), n, C.c_void_p(orig.data_ptr()),
                                         C.c_void_p(dir.data_ptr()), group, flags, None if f32 else p,
                                         p if f32 else None, _stream(stream), pst))
        return (rgb, Stats.from_c(st)) if stats else rgb

    # -- float32 radiance queries (rt_shade_rays_f32*) ------------------------
    def shade_rays_f32(self, opts: Options, orig, dir, group=1, sort=False, stats=False, stream=None):
        """shade_rays in the float32 mode's arithmetic: the colour the fp32
        render computes for a camera sample with each ray, for n
        caller-supplied rays; the scene's own camera is not read. orig and
        dir are (n, 3) float32 — numpy arrays (the host form) or CUDA torch
        tensors (the device form, enqueued on `stream`; it waits only with
        stats=True); dir as given, not normalised. Of opts bias, maxRayDepth,
        precision (fp32) and of its flags RT_FLAG_NO_BINNING are read.
        group=1: one colour per ray; group=g: the float32 sum of each run of
        g colours in index order times float32(1 / g). Returns rgb as a
        float32 (n / group, 3) array of the same kind, then the Stats when
        asked. A degenerate ray (a non-finite component, a zero direction) is
        (0, 0, 0) and counts nowhere; sort shades the rays in a coherence
        order (the same answers)."""
        flags = abi.RT_QUERY_SORT if sort else 0
        group = int(group)
        o = opts.to_c()
        st = abi.rt_stats()
        pst = C.byref(st) if stats else None
        fp = C.POINTER(C.c_float)
        if _is_host(orig):
            og, d = _host_f32(orig), _host_f32(dir)
            n = og.shape[0]
            if d.shape[0] != n:
                raise ValueError("orig and dir must hold the same number of rays")
            ng = n // group if group >= 1 and n % group == 0 else 0  # (the library reports a bad group)
            rgb = np.zeros((ng, 3), dtype=np.float32)
            check(lib().rt_shade_rays_f32(self.h, C.byref(o), n, og.ctypes.data_as(fp), d.ctypes.data_as(fp), group,
                                          flags, rgb.ctypes.data_as(fp), pst))
            return (rgb, Stats.from_c(st)) if stats else rgb
        import torch
        n = _dev_f32(orig, None)
        _dev_f32(dir, n)
        ng = n // group if group >= 1 and n % group == 0 else 0
        rgb = torch.empty((ng, 3), dtype=torch.float32, device=orig.device)
        check(lib().rt_shade_rays_f32_device(self.h, C.byref(o), n, C.c_void_p(orig.data_ptr()),
                                             C.c_void_p(dir.data_ptr()), group, flags, C.c_void_p(rgb.data_ptr()),
                                             _stream(stream), pst))
        return (rgb, Stats.from_c(st)) if stats else rgb

    def shade32_subset(self):
        """The specialisation of the float32 radiance-query kernel that
        shade_rays_f32 launches on this scene: f32_subset's feature bits
        without stochastic sampling."""
        f = lib().rtmi_test_shade32_subset
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        r = f(self.h)
        if r < 0:
            raise RuntimeError("rtmi_test_shade32_subset failed")
        return int(r)

    # -- float32 ray queries (rt_trace_rays_f32* / rt_pick_pixels_f32*) ------
    def trace_rays_f32(self, orig, dir, t_near=None, any_hit=False, sort=False, normals=False, stats=False,
                       stream=None):
        """trace_rays in the float32 mode's arithmetic: what the fp32 render's
        trace answers for n caller-supplied rays. orig and dir are (n, 3)
        float32 — numpy arrays (the host form) or CUDA torch tensors (the
        device form, enqueued on `stream`; it waits only with stats=True) —
        dir as given, not normalised; t_near (n,) float32 or None for +inf.
        Returns (t, obj, face[, normals][, Stats]) as arrays of the same
        kind, t and the normals float32: t is the ray's t_near and obj / face
        are -1 on a miss; with any_hit only obj >= 0 / obj == -1 is
        meaningful; sort traces the rays in a coherence order (the same
        answers); normals: the N the fp32 render shades the hit with,
        (0, 0, 0) on a miss. The device form's t / obj / face are views of
        one (n, 4) float32 tensor."""
        flags = (abi.RT_QUERY_ANY_HIT if any_hit else 0) | (abi.RT_QUERY_SORT if sort else 0)
        if _is_host(orig):
            o, d = _host_f32(orig), _host_f32(dir)
            n = o.shape[0]
            if d.shape[0] != n:
                raise ValueError("orig and dir must hold the same number of rays")
            tn = None if t_near is None else _host_f32n(t_near, 1)
            if tn is not None and tn.shape[0] != n:
                raise ValueError("t_near must hold one value per ray")
            return self._query_host(_HITS32, n, normals, stats, lambda hits, nrm, st: lib().rt_trace_rays_f32(
                self.h, n, _fptr(o), _fptr(d), _fptr(tn), flags, hits, nrm, st))
        n = _dev_f32(orig, None)
        _dev_f32(dir, n)
        if t_near is not None:
            _dev_f32n(t_near, n, 1)
        return self._query_device(_HITS32, orig, n, normals, stats, lambda hits, nrm, st: lib().rt_trace_rays_f32_device(
            self.h, n, C.c_void_p(orig.data_ptr()), C.c_void_p(dir.data_ptr()),
            C.c_void_p(t_near.data_ptr()) if t_near is not None else None, flags, hits, nrm, _stream(stream), st))

    def pick_f32(self, opts: Options, xy, any_hit=False, sort=False, normals=False, stats=False, stream=None):
        """What the fp32 render shows at image position xy[i] = (x, y): the
        ray that render forms for a sample there (the scene's current camera,
        an opts.width x opts.height image; opts.precision must be fp32),
        traced with t_near = +inf. Integer (x, y) is the akNone sample of
        that pixel; fractional and out-of-image positions are legal. xy is
        (n, 2) float32, numpy or CUDA torch; returns as trace_rays_f32 does,
        the Stats' numPrimaryRays counting the rays that are not degenerate."""
        flags = (abi.RT_QUERY_ANY_HIT if any_hit else 0) | (abi.RT_QUERY_SORT if sort else 0)
        o = opts.to_c()
        if _is_host(xy):
            p = _host_f32n(xy, 2)
            n = p.shape[0]
            return self._query_host(_HITS32, n, normals, stats, lambda hits, nrm, st: lib().rt_pick_pixels_f32(
                self.h, C.byref(o), n, _fptr(p), flags, hits, nrm, st))
        n = _dev_f32n(xy, None, 2)
        return self._query_device(_HITS32, xy, n, normals, stats, lambda hits, nrm, st: lib().rt_pick_pixels_f32_device(
            self.h, C.byref(o), n, C.c_void_p(xy.data_ptr()), flags, hits, nrm, _stream(stream), st))

    def trace32_subset(self):
        """The specialisation of the float32 ray-query kernel that
        trace_rays_f32 and pick_f32 launch on this scene: f32_subset's four
        geometry bits."""
        f = lib().rtmi_test_trace32_subset
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        r = f(self.h)
        if r < 0:
            raise RuntimeError("rtmi_test_trace32_subset failed")
        return int(r)

    # -- feature buffers (rt_render_aovs*) ------------------------------------
    AOV_CHANNELS = ("alpha", "depth", "object", "face", "normal", "albedo")

    def render_aovs(self, opts: Options, channels=AOV_CHANNELS, y0=0, y1=None, stream=None, stats=False,
                    host=False, out=None):
        """The per-pixel feature buffers of the fp32 frame `opts` describes,
        rows [y0, y1): a dict by channel name — alpha, depth (height, width)
        float32; object, face (height, width) int32; normal, albedo (height,
        width, 3) float32 — over the frame's own samples (include/rtmi.h
        rt_aov_buffers). CUDA torch tensors (the device form, enqueued on
        `stream`; it waits only with stats=True), or numpy arrays with
        host=True. Rows outside [y0, y1) are not written: they are zero in
        arrays made here, and keep their contents in arrays passed in `out`
        (a dict by channel name of contiguous arrays of those shapes and
        types; numpy arrays select the host form). With stats=True returns
        (dict, Stats)."""
        return self._render_aovs(opts, channels, y0, y1, stream, stats, host, out, False)

    def render_aovs_f64(self, opts: Options, channels=AOV_CHANNELS, y0=0, y1=None, stream=None, stats=False,
                        host=False, out=None):
        """The per-pixel feature buffers of the fp64 frame `opts` describes
        (include/rtmi.h rt_aov_buffers64, rt_render_aovs_f64*): render_aovs'
        arguments and results, with alpha, depth, normal and albedo float64.
        normal and albedo are summed in sample order, so every channel has
        one correct bit pattern; of opts.flags RT_FLAG_NO_BINNING and
        RT_FLAG_F64_PER_LANE are honoured and change no byte."""
        return self._render_aovs(opts, channels, y0, y1, stream, stats, host, out, True)

    def _render_aovs(self, opts, channels, y0, y1, stream, stats, host, out, f64):
        w, h = int(opts.width), int(opts.height)
        unknown = [c for c in channels if c not in self.AOV_CHANNELS]
        if unknown:
            raise ValueError(f"unknown feature buffers {unknown}: the channels are {self.AOV_CHANNELS}")
        out = dict(out or {})
        if any(_is_host(a) for a in out.values()):
            host = True
        bufs = (abi.rt_aov_buffers64 if f64 else abi.rt_aov_buffers)()
        ftype, fnp = (C.c_double, np.float64) if f64 else (C.c_float, np.float32)
        res = {}
        for c in self.AOV_CHANNELS:
            if c not in channels:
                continue
            shape = (h, w, 3) if c in ("normal", "albedo") else (h, w)
            ints = c in ("object", "face")
            ctype = C.c_int32 if ints else ftype
            a = out.get(c)
            if host:
                dt = np.int32 if ints else fnp
                if a is None:
                    a = np.zeros(shape, dtype=dt)
                elif not (_is_host(a) and a.dtype == dt and a.flags["C_CONTIGUOUS"] and a.size == int(np.prod(shape))):
                    raise ValueError(f"out[{c!r}] must be a contiguous {np.dtype(dt).name} numpy array of shape {shape}")
                ptr = a.ctypes.data_as(C.POINTER(ctype))
            else:
                import torch
                dt = torch.int32 if ints else (torch.float64 if f64 else torch.float32)
                if a is None:
                    a = torch.zeros(shape, dtype=dt, device=f"cuda:{self.device}")
                elif _is_host(a) or not (a.is_cuda and a.dtype == dt and a.is_contiguous()
                                         and a.numel() == int(np.prod(shape))):
                    raise ValueError(f"out[{c!r}] must be a contiguous {dt} CUDA/HIP tensor of shape {shape}")
                ptr = C.cast(C.c_void_p(a.data_ptr()), C.POINTER(ctype))
            setattr(bufs, c, ptr)
            res[c] = a
        o = opts.to_c()
        st = abi.rt_stats()
        pst = C.byref(st) if stats else None
        y1 = h if y1 is None else int(y1)
        if host:
            call = lib().rt_render_aovs_f64 if f64 else lib().rt_render_aovs
            check(call(self.h, C.byref(o), C.byref(bufs), int(y0), y1, pst))
        else:
            call = lib().rt_render_aovs_f64_device if f64 else lib().rt_render_aovs_device
            check(call(self.h, C.byref(o), C.byref(bufs), int(y0), y1, _stream(stream), pst))
        return (res, Stats.from_c(st)) if stats else res

    def _query_host(self, k, n, normals, stats, call):
        """The host form of a hit query in precision k (_HITS): the hits and normals made here."""
        hits = np.zeros(n, dtype=k.rec)
        nrm = np.zeros((n, 3), dtype=k.scalar) if normals else None
        st = abi.rt_stats()
        check(call(hits.ctypes.data_as(C.POINTER(k.hit)), k.ptr(nrm), C.byref(st) if stats else None))
        out = (hits["t"].copy(), hits["obj"].copy(), hits["face"].copy())
        return out + ((nrm,) if normals else ()) + ((Stats.from_c(st),) if stats else ())

    def _query_device(self, k, like, n, normals, stats, call):
        """The device form: t / obj / face are views of one (n, k.width) hit tensor."""
        import torch
        dt = getattr(torch, np.dtype(k.scalar).name)
        hits = torch.empty((n, k.width), dtype=dt, device=like.device)
        nrm = torch.empty((n, 3), dtype=dt, device=like.device) if normals else None
        st = abi.rt_stats()
        check(call(C.c_void_p(hits.data_ptr()), C.c_void_p(nrm.data_ptr()) if normals else None,
                   C.byref(st) if stats else None))
        words = hits.view(torch.int32)
        out = (hits[:, 0], words[:, k.obj], words[:, k.face])
        return out + ((nrm,) if normals else ()) + ((Stats.from_c(st),) if stats else ())

    def last_pipelined(self):
        """Whether the last render call was pipelined (its build on the
        scene's build stream, its own buffer set: rt_scene.h rt_scene::pipe) —
        such calls on two alternating streams may render at once."""
        f = lib().rtmi_test_last_pipelined
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        s = C.c_int32()
        r = f(self.h, C.byref(s))
        if r < 0:
            raise RuntimeError("rtmi_test_last_pipelined failed")
        return bool(r)

    def f32_subset(self, opts: Options):
        """The float32 kernel specialisation a render call with `opts`
        launches on this scene: the SUB_* feature bits (csrc/rt_common.h:
        sphere 1, box 2, mesh 4, general transform 8, point light 16,
        reflection 32, stochastic sampling 64)."""
        f = lib().rtmi_test_f32_subset
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(abi.rt_options)]
        o = opts.to_c()
        r = f(self.h, C.byref(o))
        if r < 0:
            raise RuntimeError("rtmi_test_f32_subset failed")
        return int(r)

    def last_split(self):
        """(lean, general) pixel groups of the last render call (two-class launches)."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().rt_scene_last_split(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_uniform(self):
        """(lit, sky): the last call's lean pixels proved uniform-lit and
        uniform-sky by its build (0, 0 when it classified nothing)."""
        a, b = C.c_int32(), C.c_int32()
        check(lib().rt_scene_last_uniform(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_ground(self):
        """The last call's general pixels its build tagged as ground pixels
        (0 when it tagged nothing)."""
        a = C.c_int32()
        check(lib().rt_scene_last_ground(self.h, C.byref(a)))
        return int(a.value)

    def last_mesh1(self):
        """The last call's batches of mesh-pixel samples that took the
        one-plane batched kernel's straight path (0 when none could: see
        RT_FLAG_NO_MESH1). Valid once the call's Stats have been read."""
        a = C.c_int64()
        check(lib().rt_scene_last_mesh1(self.h, C.byref(a)))
        return int(a.value)

    def last_lean_kernel(self):
        """Kernels of the last call's two classes: bits 0-1 the lean pixels'
        (0 none, 1 k_render_lean, 2 k_render_lean1q, 3 merged), bits 2-3 the
        general pixels' (0 k_render_fast, 1 k_render_gen, 2 k_render_gen1,
        3 merged: k_render_mix1)."""
        k = C.c_int32()
        check(lib().rt_scene_last_lean_kernel(self.h, C.byref(k)))
        return int(k.value) & 15

    def last_compacted(self):
        """Whether the last call traced its reflected rays in per-wave
        compacted passes (k_render_wave; reflective scenes with RT_FLAG_COMPACT)."""
        k = C.c_int32()
        check(lib().rt_scene_last_lean_kernel(self.h, C.byref(k)))
        return bool(int(k.value) & 16)

    def last_lean_lanes(self):
        """Lanes per lean pixel of the last two-class call (4 or 16:
        k_render_lean1q / k_render_mix1; 64: k_render_lean, one pixel per
        wave), 0 if none."""
        k = C.c_int32()
        check(lib().rt_scene_last_lean_kernel(self.h, C.byref(k)))
        return int(k.value) >> 8

    def last_batch(self):
        """(batched, fallback) general pixel groups of the last render call:
        those the batched general kernel took, and of them those it
        re-rendered with the one-sample loop (as of the last call with Stats)."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().rt_scene_last_batch(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_timing(self):
        """(setup_ms, render_ms) of the last call made with RT_FLAG_TIMING:
        its per-call camera-dependent build and its render kernels (waits)."""
        a, b = C.c_double(), C.c_double()
        check(lib().rt_scene_last_timing(self.h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def last_counters(self):
        c = abi.rt_traversal_counters()
        check(lib().rt_scene_last_counters(self.h, C.byref(c)))
        return c.as_dict()


def band_rows(height, band_h, world):
    out = C.c_int32()
    check(lib().rt_band_rows(int(height), int(band_h), int(world), C.byref(out)))
    return out.value


def unshard_bands_device(d_gathered, d_fb, width, height, band_h, world, stream=None):
    rows = band_rows(height, band_h, world)
    check(lib().rt_unshard_bands_device(C.c_void_p(_ptr(d_gathered, world * rows * width * 3)),
                                        C.c_void_p(_ptr(d_fb, width * height * 3)), int(width),
                                        int(height), int(band_h), int(world), _stream(stream)))


def _object_kinds(arr, n):
    """(type, mesh) of every object of a flattened list: what an object
    update must keep."""
    return [(int(arr[i].type), int(arr[i].mesh)) for i in range(n)]


def _checked_objects(objs, mesh_ids, kinds):
    """The rt_object_desc array of `objs` for an update of a device scene
    created with `kinds`; ValueError / TypeError when the count, a kind or a
    mesh differs."""
    if len(objs) != len(kinds):
        raise ValueError(f"the device scene has {len(kinds)} objects, not {len(objs)}: set_objects keeps the count")
    arr, _ = flatten_objects(objs, mesh_ids)
    for i, (have, want) in enumerate(zip(_object_kinds(arr, len(objs)), kinds)):
        if have[0] != want[0]:
            raise TypeError(f"object {i}: its kind differs from the one the device scene was created with")
        if have[1] != want[1]:
            raise ValueError(f"object {i}: its mesh differs from the one the device scene was created with")
    return arr


def _shape_key(scene: Scene):
    """What the device copy holds of a Scene that no in-place edit replaces:
    the objects' kinds, sphere radii, the FULL box bounds (all of vmin / vmax,
    geom.nim:169-170), mesh identity and sizes, background — the fingerprint
    INTEGRATION.md's Nim binding (shapeHash) keeps; a change rebuilds the
    device scene. The camera, the lights (_lights_key) and the objects'
    transforms and materials (_pose_key) are pushed to the copy instead. Mesh
    vertices edited in place (same sizes) are not hashed per call: updateMesh
    (or invalidateScene, which rebuilds)."""
    from .scene import Box, Sphere, TriangleMesh
    parts = []
    for o in scene.objects:
        g = o.geometry
        parts.append(type(g).__name__)
        if isinstance(g, Sphere):
            parts.append(g.r)
        elif isinstance(g, Box):
            parts += [g.vmin.tobytes(), g.vmax.tobytes()]
        elif isinstance(g, TriangleMesh):
            parts += [id(g), g.vertices.shape[0], g.faces.shape[0], id(g.vertices), id(g.faces)]
    parts.append(np.asarray(scene.bgColor, np.float64).tobytes())
    return tuple(parts)


def _pose_key(scene: Scene):
    """Where every object stands and what it is made of (the Nim binding's
    poseHash): a change is pushed to the existing device copy
    (rt_scene_set_objects)."""
    parts = []
    for o in scene.objects:
        g = o.geometry
        parts += [np.asarray(g.objectToWorld, np.float64).tobytes(),
                  np.asarray(g.worldToObject, np.float64).tobytes(),
                  np.asarray(o.material.albedo, np.float64).tobytes(), float(o.material.reflection)]
    return tuple(parts)


def _lights_key(scene: Scene):
    """The lights' fingerprint (the Nim binding's lightsHash): a change is
    pushed to the existing device copy (rt_scene_set_lights)."""
    from .scene import DistantLight
    parts = []
    for li in scene.lights:
        parts += [type(li).__name__, np.asarray(li.color, np.float64).tobytes(), float(li.intensity),
                  np.asarray(li.dir if isinstance(li, DistantLight) else li.pos, np.float64).tobytes()]
    return tuple(parts)


class _Entry:
    """One cached device copy: the DeviceScene, what it was built from, and
    the renderLine calls running on it (renders happen outside the cache's
    lock, so a replaced or invalidated copy is closed by whichever comes
    last: the replacement, or the last of those calls)."""
    __slots__ = ("ds", "shape", "pose", "lights", "cam", "fov", "users", "retired")

    def __init__(self, ds, shape, pose, lights, cam, fov):
        self.ds, self.shape, self.pose, self.lights, self.cam, self.fov = ds, shape, pose, lights, cam, fov
        self.users = 0
        self.retired = False


class _DeviceCache:
    """The Nim binding's `deviceScene` in Python: one device
    copy per Scene, created on first use, re-created when the shape key
    changes, its objects' transforms and materials pushed
    (rt_scene_set_objects) when they moved, its lights pushed
    (rt_scene_set_lights) when only Scene.lights changed, its camera pushed (rt_scene_set_camera) when Scene.cameraToWorld
    / fov moved — renderLine re-reads them on every call (renderer.nim:135-136,
    150-153). Re-entrant like renderLine (the pool calls it from
    countProcessors() threads at once, workerpool.nim:72-99): lookups,
    creation and camera pushes hold one lock; the render call itself runs
    outside it (the library serialises calls per scene), counted in its
    entry, and a copy that is replaced or invalidated meanwhile is destroyed
    only once its last call has returned (no use after free). Entries are
    keyed weakly: when a Scene is collected, its device copy is released
    (the cache no longer keeps every Scene and its GPU buffers
    alive)."""

    def __init__(self):
        # re-entrant: a Scene collected while this thread holds the lock runs
        # its weakref callback (_collected) on this thread
        self._lock = threading.RLock()
        self._entries = {}  # id(scene) -> (weakref to the scene, _Entry)

    def _drop(self, e):
        # under the lock: retire e; close it now if no call is running on it
        e.retired = True
        return e.ds if e.users == 0 else None

    def acquire(self, scene: Scene, device=0):
        """(DeviceScene, entry) with the entry's call count raised; pass the
        entry to release() when the call has returned."""
        import weakref
        shape = _shape_key(scene)
        pose = _pose_key(scene)
        lights = _lights_key(scene)
        cam = np.asarray(scene.cameraToWorld, np.float64).tobytes()
        fov = float(scene.fov)
        stale = None
        with self._lock:
            key = id(scene)
            item = self._entries.get(key)
            e = item[1] if item is not None and item[0]() is scene else None
            if e is not None and e.shape != shape:  # kinds, sizes or meshes changed
                stale = self._drop(e)
                e = None
            if e is None:
                ds = DeviceScene(scene, device)
                ds.scene = weakref.proxy(scene)  # the cache must not keep the Scene alive
                e = _Entry(ds, shape, pose, lights, cam, fov)
                self._entries[key] = (weakref.ref(scene, lambda _r, k=key: self._collected(k)), e)
            else:
                if e.pose != pose:  # objects moved or restyled: the copy takes them, nothing is rebuilt
                    e.ds.set_objects(scene.objects)
                    e.pose = pose
                if e.lights != lights:  # only the lights changed: the copy is relit, not rebuilt
                    e.ds.set_lights(scene.lights)
                    e.lights = lights
                if e.cam != cam or e.fov != fov:  # the camera moved: the next call renders it
                    e.ds.set_camera(scene.cameraToWorld, fov)
                    e.cam, e.fov = cam, fov
            e.users += 1
        if stale is not None:
            stale.close()
        return e.ds, e

    def release(self, e):
        with self._lock:
            e.users -= 1
            last = e.retired and e.users == 0
        if last:
            e.ds.close()

    def get(self, scene: Scene, device=0) -> "DeviceScene":
        """The device copy, NOT held: for single-threaded callers that keep
        it in step with invalidate() themselves. A concurrent
        invalidateScene, shape change or collection of the Scene may close
        the returned copy while it is in use; threaded callers use held()
        (or renderLine, which holds the copy for each call)."""
        ds, e = self.acquire(scene, device)
        self.release(e)
        return ds

    @contextlib.contextmanager
    def held(self, scene: Scene, device=0):
        """`with held(scene) as ds:` the device copy, kept open until the
        block ends (acquire / release around it) even if another thread
        invalidates or replaces it meanwhile."""
        ds, e = self.acquire(scene, device)
        try:
            yield ds
        finally:
            self.release(e)

    def invalidate(self, scene: Scene):
        with self._lock:
            item = self._entries.pop(id(scene), None)
            stale = self._drop(item[1]) if item is not None else None
        if stale is not None:
            stale.close()

    def update_mesh(self, scene: Scene, mesh):
        """Push `mesh`'s current vertices (and normals) to the cached device
        copy, if there is one: the copy and its handle stay, nothing is
        rebuilt. Without a copy the next acquire creates from current data."""
        with self._lock:
            item = self._entries.get(id(scene))
            e = item[1] if item is not None and item[0]() is scene else None
            if e is not None and not e.retired:
                e.ds.set_mesh_vertices(mesh, mesh.vertices, mesh.normals)

    def _collected(self, key):
        with self._lock:
            item = self._entries.get(key)
            if item is None or item[0]() is not None:
                return
            del self._entries[key]
            stale = self._drop(item[1])
        if stale is not None:
            stale.close()

    def __len__(self):
        with self._lock:
            return len(self._entries)


_cache = _DeviceCache()


def deviceScene(scene: Scene, device=0) -> "DeviceScene":
    """The cached device copy of `scene` (INTEGRATION.md deviceScene).
    Single-threaded use only: the copy is not held (see heldDeviceScene)."""
    return _cache.get(scene, device)


def heldDeviceScene(scene: Scene, device=0):
    """Context manager: the cached device copy of `scene`, held open for the
    block (safe against a concurrent invalidateScene / Scene edit)."""
    return _cache.held(scene, device)


def invalidateScene(scene: Scene):
    """After editing mesh faces in place (same sizes): the device copy is
    rebuilt by the next call. For vertices alone updateMesh is far cheaper."""
    _cache.invalidate(scene)


def updateMesh(scene: Scene, mesh):
    """After editing `mesh.vertices` (one of scene's TriangleMesh objects) in
    place: the cached device copy takes the new positions
    (rt_scene_set_mesh_vertices: records, normals, a BVH refit and the light
    grids on the device) and keeps its handle."""
    _cache.update_mesh(scene, mesh)


def renderLine(scene, opts: Options, fb, y, step=1, maxStep=1) -> Stats:
    """renderer.nim:162-211 — one scanline (and its step x step blocks).
    `scene` is the reference's Scene (its device copy is cached and kept in
    step with the Scene's camera, as the Nim binding does) or a DeviceScene."""
    if isinstance(scene, DeviceScene):
        return scene.render_lines(opts, fb, y, y + 1, step, maxStep)
    ds, e = _cache.acquire(scene)
    try:
        return ds.render_lines(opts, fb, y, y + 1, step, maxStep)
    finally:
        _cache.release(e)


def render_frame(scene: DeviceScene, opts: Options, fb=None):
    """Whole frame through the host-framebuffer path. Returns (fb, Stats)."""
    if fb is None:
        fb = np.zeros((opts.height, opts.width, 3), dtype=np.float32)
    st = scene.render_lines(opts, fb, 0, opts.height, 1, 1)
    return fb, st


def ppm_encode_device(d_fb, width, height, bits=8, sRGB=True, stream=None):
    """writePpm's payload (framebuf.nim:55-93) of a device framebuffer,
    quantised on the GPU; returns (header bytes, uint8 CUDA tensor)."""
    import torch
    n = lib().rt_ppm_payload_bytes(int(width), int(height), int(bits))
    if n < 0:
        raise RtmiError(n, lib().rt_last_error().decode())
    out = torch.empty(n, dtype=torch.uint8, device=d_fb.device)
    check(lib().rt_ppm_encode_device(C.c_void_p(_ptr(d_fb, width * height * 3)), int(width), int(height),
                                     int(bits), 1 if sRGB else 0, C.c_void_p(int(out.data_ptr())),
                                     _stream(stream)))
    buf = C.create_string_buffer(64)
    hl = lib().rt_ppm_header(int(width), int(height), int(bits), buf, 64)
    if hl < 0:
        raise RtmiError(hl, lib().rt_last_error().decode())
    return buf.raw[:hl], out


class MultiDeviceScene:
    """One process, several GPUs (rt_multi_*, SURVEY.md 8(b)
    rt_render_frame_multi): the scene replicated on every listed device
    (repeats allowed), bands dealt round-robin, gathered on devices[0]."""

    def __init__(self, scene: Scene, devices=(0,), band_h=4):
        initRenderer(devices[0])
        self.devices = list(devices)
        flat = flatten(scene)
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        h = C.c_void_p()
        check(lib().rt_multi_create(C.byref(flat.desc), arr, len(self.devices), int(band_h), C.byref(h)))
        self.h = h
        self._mesh_ids = [id(g) for g in flat._meshes]
        self._kinds = _object_kinds(flat._objs, len(scene.objects))

    def set_camera(self, cameraToWorld, fov):
        """rt_scene_set_camera on every rank's scene."""
        arr = (C.c_double * 16)(*[float(x) for x in glm.flat(cameraToWorld)])
        check(lib().rt_multi_set_camera(self.h, arr, float(fov)))

    def set_lights(self, lights):
        """rt_scene_set_lights on every rank's scene."""
        ls = list(lights)
        check(lib().rt_multi_set_lights(self.h, flatten_lights(ls), len(ls)))

    def set_objects(self, objects):
        """rt_scene_set_objects on every rank's scene (DeviceScene.set_objects)."""
        objs = list(objects)
        arr = _checked_objects(objs, self._mesh_ids, self._kinds)
        check(lib().rt_multi_set_objects(self.h, arr, len(objs)))

    def set_mesh_vertices(self, mesh, vertices, normals=None):
        """rt_scene_set_mesh_vertices on every rank's scene (host arrays);
        `mesh` is an index or one of the Scene's TriangleMesh objects."""
        if not isinstance(mesh, (int, np.integer)):
            mesh = self._mesh_ids.index(id(mesh))
        v = _host_f64(vertices, (-1, 3))
        n = None if normals is None else _host_f64(normals, (-1, 3))
        check(lib().rt_multi_set_mesh_vertices(self.h, int(mesh), _dptr(v), v.shape[0], _dptr(n)))

    def render_frame(self, opts: Options, fb) -> Stats:
        """Whole frame into a host (h, w, 3) float32 array."""
        if not (isinstance(fb, np.ndarray) and fb.dtype == np.float32 and fb.flags.c_contiguous
                and fb.shape == (opts.height, opts.width, 3)):
            raise ValueError("fb must be a C-contiguous float32 array of shape (height, width, 3)")
        o = opts.to_c()
        st = abi.rt_stats()
        check(lib().rt_render_frame_multi(self.h, C.byref(o), fb.ctypes.data_as(C.POINTER(C.c_float)),
                                          opts.width, opts.height, C.byref(st)))
        return Stats.from_c(st)

    def render_frame_device(self, opts: Options, d_fb) -> Stats:
        """Whole frame into a device buffer on devices[0]; waits, returns Stats."""
        ptr = _ptr(d_fb, opts.width * opts.height * 3)
        o = opts.to_c()
        st = abi.rt_stats()
        check(lib().rt_render_frame_multi_device(self.h, C.byref(o), C.c_void_p(ptr), C.byref(st)))
        return Stats.from_c(st)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().rt_multi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResponseMsg:
    """ResponseMsg (raytracer.nim:21-23) plus the line it answers."""

    def __init__(self, line, stats):
        self.line = line
        self.stats = stats


class RenderQueue:
    """WorkerPool[WorkMsg, ResponseMsg] (src/concurrency/workerpool.nim) as
    raytracer.nim / gui.nim drive it, over the GPU (rt_queue_*): queued
    lines that form a run at one step become one launch; every line gets its
    response; a run's Stats ride on its last response (callers sum them)."""

    numActiveWorkers = 1  # one device "worker"; the pool size has no GPU meaning
    poolSize = 1

    def __init__(self, ds: DeviceScene):
        self.ds = ds
        h = C.c_void_p()
        check(lib().rt_queue_create(ds.h, C.byref(h)))
        self.h = h
        self._fbs = {}  # framebuffers the queue's thread may still write

    def state(self):
        return lib().rt_queue_state(self.h)

    def isReady(self):
        return lib().rt_queue_is_ready(self.h) == 1

    def waitForReady(self, timeout=1):
        """Commands complete before they return: always ready."""

    def start(self):
        return lib().rt_queue_start(self.h) == 1

    def stop(self):
        return lib().rt_queue_stop(self.h) == 1

    def queueWork(self, opts: Options, framebuf, line, step=0, maxStep=0):
        """WorkMsg{opts, framebuf, line, step, maxStep}: framebuf is the
        (h, w, 3) float32 array the line is rendered into."""
        if not (isinstance(framebuf, np.ndarray) and framebuf.dtype == np.float32 and framebuf.flags.c_contiguous
                and framebuf.shape == (opts.height, opts.width, 3)):
            raise ValueError("framebuf must be a C-contiguous float32 array of shape (height, width, 3)")
        o = opts.to_c()
        check(lib().rt_queue_work(self.h, C.byref(o), framebuf.ctypes.data_as(C.POINTER(C.c_float)),
                                  opts.width, opts.height, int(line), int(step), int(maxStep)))
        self._fbs[framebuf.ctypes.data] = framebuf

    def tryRecvResult(self):
        """(available, ResponseMsg); a failed line raises RtmiError."""
        r = abi.rt_response()
        n = lib().rt_queue_try_recv(self.h, C.byref(r))
        if n < 0:
            raise RtmiError(n, lib().rt_last_error().decode())
        if n == 0:
            return False, None
        if r.status != 0:
            raise RtmiError(r.status, r.error.decode(errors="replace"))
        if lib().rt_queue_pending(self.h) == 0:
            self._fbs.clear()
        return True, ResponseMsg(r.line, Stats.from_c(r.stats))

    def reset(self):
        return lib().rt_queue_reset(self.h) == 1

    def shutdown(self):
        return lib().rt_queue_shutdown(self.h) == 1

    def close(self):
        """workerpool.nim close: only after shutdown."""
        if self.h is None or self.state() != abi.RT_QUEUE_SHUTDOWN:
            return False
        check(lib().rt_queue_destroy(self.h))
        self.h = None
        self._fbs.clear()
        return True

    def __del__(self):
        try:
            if self.h is not None:
                lib().rt_queue_destroy(self.h)
                self.h = None
        except Exception:
            pass


def initRenderWorkers(ds: DeviceScene, numActiveWorkers=0, poolSize=0):
    """initRenderWorkers (raytracer.nim:35-38) -> a RenderQueue."""
    return RenderQueue(ds)


def rgba_encode_device(d_fb, width, height, alpha=0xFF, stream=None):
    """ImageRGBA.copyFrom (image.nim:45-54) of a device framebuffer on the
    GPU; returns a (height, width, 4) uint8 CUDA tensor."""
    import torch
    out = torch.empty((int(height), int(width), 4), dtype=torch.uint8, device=d_fb.device)
    check(lib().rt_rgba_encode_device(C.c_void_p(_ptr(d_fb, width * height * 3)), int(width), int(height),
                                      int(alpha) & 0xFF, C.c_void_p(int(out.data_ptr())), _stream(stream)))
    return out


def write_ppm_device(d_fb, width, height, filename, bits=8, sRGB=True, stream=None):
    """Framebuf.writePpm for a device framebuffer: the quantisation runs on
    the GPU and only the 8/16-bit payload crosses PCIe."""
    header, payload = ppm_encode_device(d_fb, width, height, bits, sRGB, stream)
    try:
        with open(filename, "wb") as f:
            f.write(header)
            f.write(payload.cpu().numpy().tobytes())
        return True
    except OSError:
        return False


def _ptr(buf, min_floats):
    if isinstance(buf, int):
        return buf
    try:  # torch tensor
        import torch  # noqa: F401
        if not buf.is_cuda or buf.dtype.itemsize != 4 or not buf.is_contiguous():
            raise ValueError("device buffer must be a contiguous 4-byte CUDA/HIP tensor")
        if buf.numel() < min_floats:
            raise ValueError(f"device buffer holds {buf.numel()} floats, need {min_floats}")
        return int(buf.data_ptr())
    except AttributeError:
        raise TypeError("device buffer must be an int pointer or a torch tensor") from None


# rt_hit (include/rtmi.h) as a numpy record
_HIT_DTYPE = np.dtype([("t", np.float64), ("obj", np.int32), ("face", np.int32)])
# rt_hit32 likewise
_HIT32_DTYPE = np.dtype([("t", np.float32), ("obj", np.int32), ("face", np.int32), ("reserved", np.int32)])


def _is_host(a):
    """numpy (or a plain sequence): the host form; a CUDA torch tensor: the device form."""
    return not hasattr(a, "data_ptr")


def _host_f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))


def _host_f32(a):
    """(n, 3) float32 rays; another dtype is refused (no silent rounding of float64 rays)."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise ValueError(f"float32 rays expected, got {a.dtype}")
    return np.ascontiguousarray(a.reshape(-1, 3))


def _dev_f32(t, n):
    """Check a device array of n (or any number of) float32 rays; returns the ray count."""
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("device arrays must be contiguous float32 CUDA/HIP tensors")
    if t.numel() % 3 or (n is not None and t.numel() != n * 3):
        raise ValueError(f"device array holds {t.numel()} floats, expected "
                         f"{'a multiple of 3' if n is None else n * 3}")
    return t.numel() // 3


def _host_f32n(a, width):
    """(n, width) float32 rows ((n,) for width 1); another dtype is refused."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise ValueError(f"float32 values expected, got {a.dtype}")
    return np.ascontiguousarray(a.reshape(-1) if width == 1 else a.reshape(-1, width))


def _dev_f32n(t, n, width):
    """Check a device array of n (or any number of) rows of `width` float32; returns the row count."""
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("device arrays must be contiguous float32 CUDA/HIP tensors")
    if t.numel() % width or (n is not None and t.numel() != n * width):
        raise ValueError(f"device array holds {t.numel()} floats, expected "
                         f"{'a multiple of ' + str(width) if n is None else n * width}")
    return t.numel() // width


def _fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


# A hit query's arrays in each precision: the numpy record and the ABI struct
# of a hit, the scalar type of t and the normals with its pointer maker, and
# the device form's hit tensor: its width in scalars and the 32-bit word
# columns of obj / face.
_HITS64 = SimpleNamespace(rec=_HIT_DTYPE, hit=abi.rt_hit, scalar=np.float64, ptr=_dptr, width=2, obj=2, face=3)
_HITS32 = SimpleNamespace(rec=_HIT32_DTYPE, hit=abi.rt_hit32, scalar=np.float32, ptr=_fptr, width=4, obj=1, face=2)


def _dev_f64(t, n, width):
    """Check a device array of n (or any number of) rows of `width` float64; returns the row count."""
    import torch
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError("device arrays must be contiguous float64 CUDA/HIP tensors")
    if t.numel() % width or (n is not None and t.numel() != n * width):
        raise ValueError(f"device array holds {t.numel()} doubles, expected "
                         f"{'a multiple of ' + str(width) if n is None else n * width}")
    return t.numel() // width


def _stream(stream):
    """hipStream_t for the C-ABI. None = the current torch stream when torch
    is loaded (so torch ops and renders are ordered), else HIP's null stream."""
    if stream is None:
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
            return C.c_void_p(int(torch.cuda.current_stream().cuda_stream) or None)
        return None
    if isinstance(stream, int):
        return C.c_void_p(stream or None)
    return C.c_void_p(int(stream.cuda_stream) or None)


__all__ = ["DeviceScene", "RtmiError", "band_rows", "device_count", "deviceScene", "heldDeviceScene", "initRenderer", "invalidateScene",
           "ppm_encode_device", "renderLine", "render_frame", "unshard_bands_device", "updateMesh", "write_ppm_device"]

"""A sequence's depth fused into one truncated-signed-distance (TSDF) volume (include/sde_hip.h: sde_pose_compose, sde_tsdf_integrate,
sde_tsdf_points; csrc/volume.hip).  `TsdfVolume` owns the three device arrays and binds the kernels; `compose_host`, `integrate_host` and
`points_host` are their host twins -- the same fp32 operations in the same order in numpy, for machines without a GPU and for the tests,
which compare the two bit for bit.  Every frame's depth is averaged into the voxel grid through its world-to-camera pose; the zero crossings
of the grid are the surface, handed out as the 16-byte records of hip.cloud (as_records and the PLY writer take them as they are), or connected
into a triangle mesh by surface nets (sde_tsdf_mesh: `TsdfVolume.mesh`, `save_mesh`, the twin `mesh_host`, `write_mesh_ply` / `read_mesh_ply`), or
seen from a camera pose by ray casting (sde_tsdf_render: `TsdfVolume.render`, the twin `render_host`); `TsdfVolume.track` aligns a frame's depth
with that view (hip/align.py: sde_frame_align)."""
import ctypes
import warnings

import numpy as np
import torch

from . import args as A
from . import lib as L
from . import present as HP
from .cloud import RECORD, as_records
from .twins import nearest_pixel_np, pinhole_move_project_np

MAX_DIM, MAX_VOXELS = 1024, 1 << 30
DEFAULT_CAP = 1 << 22           # records `points` makes room for when the caller names no cap (64 MiB), or 3 per voxel if that is fewer


def check_params(dims, voxel, origin=None, trunc=None, max_weight=64.0, min_depth=0.0, max_depth=80.0):
    """The argument errors the C side refuses, raised as ValueError before anything touches the device.  -> (dims, voxel, origin, trunc,
    max_weight, min_depth, max_depth) as the kernels receive them (fp32 values as Python floats); origin=None puts the first camera at the
    middle of the near face, (-nx * voxel / 2, -ny * voxel / 2, 0), trunc=None is 4 * voxel."""
    try:
        given = tuple(dims)
        exact = len(given) == 3 and all(int(n) == n for n in given)
        dims = tuple(int(n) for n in given)
    except (TypeError, ValueError):
        exact = False
    if not exact or not all(1 <= n <= MAX_DIM for n in dims) or dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise ValueError(f"TsdfVolume: dims must be three integers in [1, {MAX_DIM}] with a product of at most 2^30, got {dims!r}")
    f = lambda x: float(np.float32(x))
    voxel = f(voxel)
    if not voxel > 0.0 or not np.isfinite(voxel):
        raise ValueError(f"TsdfVolume: voxel must be positive and finite, got {voxel!r}")
    trunc = f(4.0 * voxel if trunc is None else trunc)
    max_weight = f(max_weight)
    if not trunc > 0.0 or not max_weight > 0.0:
        raise ValueError(f"TsdfVolume: trunc and max_weight must be positive, got ({trunc!r}, {max_weight!r})")
    min_depth, max_depth = f(min_depth), f(max_depth)
    if not min_depth < max_depth:
        raise ValueError(f"TsdfVolume: min_depth must lie below max_depth, got ({min_depth}, {max_depth})")
    if origin is None:
        origin = (-dims[0] * voxel / 2, -dims[1] * voxel / 2, 0.0)
    origin = tuple(f(o) for o in np.asarray(origin, dtype=np.float64).reshape(-1))
    if len(origin) != 3 or not all(np.isfinite(o) for o in origin):
        raise ValueError(f"TsdfVolume: origin must be three finite numbers, got {origin!r}")
    return dims, voxel, origin, trunc, max_weight, min_depth, max_depth


def check_min_weight(min_weight):
    min_weight = float(np.float32(min_weight))
    if not min_weight >= 1.0:
        raise ValueError(f"TsdfVolume: min_weight must be at least 1, got {min_weight!r}")
    return min_weight


MAX_SAMPLES, MAX_PICTURE = 65536, 32768


def check_render(size, near, far, step):
    """The argument errors sde_tsdf_render refuses, raised as ValueError before anything touches the device.  -> (H, W, near, step, n): near and
    step as the kernel receives them (fp32 values as Python floats) and the sample count n = ceil((far - near) / step), from the fp32 values."""
    try:
        H, W = (int(s) for s in size)
        exact = len(tuple(size)) == 2 and all(int(s) == s for s in size)
    except (TypeError, ValueError):
        exact = False
    if not exact or not (1 <= H <= MAX_PICTURE and 1 <= W <= MAX_PICTURE):
        raise ValueError(f"TsdfVolume.render: size must be (H, W), integers in [1, {MAX_PICTURE}], got {size!r}")
    near, far, step = (float(np.float32(x)) for x in (near, far, step))
    if not (np.isfinite(near) and np.isfinite(far) and np.isfinite(step)) or not step > 0.0:
        raise ValueError(f"TsdfVolume.render: near and far must be finite, step positive and finite, got ({near!r}, {far!r}, {step!r})")
    n = int(np.ceil((far - near) / step))
    if not 1 <= n <= MAX_SAMPLES:
        raise ValueError(f"TsdfVolume.render: ceil((far - near) / step) samples must lie in [1, {MAX_SAMPLES}], got {n} (near {near}, far {far}, step {step})")
    return H, W, near, step, n


def pose_compose(T, C):
    """C <- T C in place: T, C [4,4] (or [1,4,4]) fp32 contiguous CUDA tensors, one rigid transform each.  One launch, no host synchronisation."""
    dev = C.device if torch.is_tensor(C) else None
    for what, t in (("C", C), ("T", T)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != 16 or tuple(t.shape[-2:]) != (4, 4) or t.device != dev:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise L.SdeHipError(f"pose_compose: {what} must be one float32 [4,4] tensor on {dev}, got {got}")
    L.check(L.lib().sde_pose_compose(L.ptr(T), L.ptr(C), L.stream()), "sde_pose_compose")
    return C


class TsdfVolume:
    """nx x ny x nz voxels of edge `voxel`, x fastest: `tsdf` and `weight` [nz,ny,nx] fp32 and, with colour, `rgba` [nz,ny,nx,4] uint8 on
    `device`.  Extents are in the units of the depth that is integrated (a monocular model's depth is known up to one scale factor)."""

    def __init__(self, dims, voxel, origin=None, trunc=None, max_weight=64.0, min_depth=0.0, max_depth=80.0, colour=True, device="cuda"):
        self.dims, self.voxel, self.origin, self.trunc, self.max_weight, self.min_depth, self.max_depth = check_params(
            dims, voxel, origin, trunc, max_weight, min_depth, max_depth)
        self.colour = bool(colour)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SdeHipError("TsdfVolume: the volume lives on a GPU; there is no CPU fallback (the host twins are functions of this module)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        nx, ny, nz = self.dims
        self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.rgba = torch.empty((nz, ny, nx, 4), dtype=torch.uint8, device=self.device) if self.colour else None
        self._origin = (ctypes.c_float * 3)(*self.origin)
        self.reset()

    def params(self):
        """What a captured launch depends on: the parameters and the addresses of ALL the arrays (a later volume may get one array of an earlier
        one back from the allocator and the others elsewhere)."""
        return (self.dims, self.voxel, self.origin, self.trunc, self.max_weight, self.min_depth, self.max_depth, self.colour, self.tsdf.data_ptr(),
                self.weight.data_ptr(), self.rgba.data_ptr() if self.rgba is not None else 0)

    def reset(self):
        """A fresh volume, on the current stream: tsdf = 1, weight = 0, rgba = 0."""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.rgba is not None:
            self.rgba.zero_()

    def integrate(self, pred, ymap, xmap, K, C, frame=None):
        """One frame into the volume.  pred [ph,pw] (or [1,ph,pw] / [1,1,ph,pw]) fp32, ymap [H] / xmap [W] int32 (hip.present's maps), K [3,3]
        fp32 at the restored size, C [4,4] fp32 world -> camera, frame [H,W,3] uint8 or None (no colour): CUDA tensors on the volume's device.
        One launch on the current stream, no host synchronisation (device maps: see depth_present)."""
        pred = A.as_pred("tsdf_integrate", pred)
        A.same_device_tensor("tsdf_integrate", "pred", pred, torch.float32, (1, None, None), self.device)
        _, ph, pw = pred.shape
        ymap, xmap = HP.ensure_checked(ymap, xmap, ph, pw, self.device)
        H, W = ymap.numel(), xmap.numel()
        K = A.as_K("tsdf_integrate", K, 1, self.device)
        if torch.is_tensor(C) and C.dim() == 3:
            C = C[0]
        C = A.same_device_tensor("tsdf_integrate", "C", C, torch.float32, (4, 4), self.device)
        frame = A.as_frame("tsdf_integrate", frame, 1, H, W, self.device)
        nx, ny, nz = self.dims
        L.check(L.lib().sde_tsdf_integrate(L.ptr(pred), ph, pw, L.ptr(ymap), L.ptr(xmap), H, W, L.ptr(frame), L.ptr(K), L.ptr(C), self._origin, self.voxel,
                                           self.trunc, self.max_weight, self.min_depth, self.max_depth, L.ptr(self.tsdf), L.ptr(self.weight),
                                           L.ptr(self.rgba), nx, ny, nz, L.stream()), "sde_tsdf_integrate")

    def compose(self, T, C):
        """C <- T C in place (pose_compose): the world-to-camera pose advanced by the step T, frame i -> frame i + 1."""
        return pose_compose(T, C)

    def default_cap(self):
        return min(3 * self.dims[0] * self.dims[1] * self.dims[2], DEFAULT_CAP)

    def workspace_numel(self):
        """int32 elements of workspace sde_tsdf_points asks for."""
        return int(L.lib().sde_tsdf_points_ws_bytes(*self.dims)) // 4

    def points(self, min_weight=1, cap=None, out=None, workspace=None):
        """The zero crossings between voxels of weight >= min_weight -> (points [cap,16] uint8, count [1] int32) on the device: the records are
        points[:min(count, cap)], ascending voxel then axis (hip.cloud.as_records gives the structured view); count is the total, also when it
        exceeds cap.  cap=None: default_cap().  out: optional (points, count) destinations; workspace: optional int32 tensor of at least
        workspace_numel() elements.  Three launches on the current stream, no host synchronisation."""
        min_weight = check_min_weight(min_weight)
        cap = self.default_cap() if cap is None else int(cap)
        if not 1 <= cap <= 0x7fffffff:
            raise ValueError(f"TsdfVolume.points: cap must lie in [1, 2^31), got {cap}")
        points, count = out if out is not None else (None, None)
        points = A.dst("tsdf_points", points, (cap, 16), torch.uint8, True, self.device)
        count = A.dst("tsdf_points", count, (1,), torch.int32, True, self.device)
        need = self.workspace_numel()
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.int32, device=self.device)
        if workspace.dtype != torch.int32 or workspace.device != self.device:
            raise L.SdeHipError(f"tsdf_points: workspace must be an int32 tensor on {self.device}, got {workspace.dtype} on {workspace.device}")
        nx, ny, nz = self.dims
        L.check(L.lib().sde_tsdf_points(L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(self.rgba), nx, ny, nz, self._origin, self.voxel, min_weight,
                                        L.ptr(workspace), workspace.numel() * 4, L.ptr(points), cap, L.ptr(count), L.stream()), "sde_tsdf_points")
        return points, count

    def default_mesh_caps(self):
        """(cap_vertices, cap_faces) `mesh` makes room for when the caller names none: every cell a vertex and six triangles, or DEFAULT_CAP
        vertices (64 MiB) and twice as many triangles (96 MiB) if that is fewer."""
        cells = max((self.dims[0] - 1) * (self.dims[1] - 1) * (self.dims[2] - 1), 1)
        return min(cells, DEFAULT_CAP), min(6 * cells, 2 * DEFAULT_CAP)

    def mesh_workspace_numel(self):
        """int32 elements of workspace sde_tsdf_mesh asks for."""
        return int(L.lib().sde_tsdf_mesh_ws_bytes(*self.dims)) // 4

    def mesh(self, min_weight=1, cap_vertices=None, cap_faces=None, out=None, workspace=None):
        """The surface as triangles (surface nets: one vertex per cell that holds a crossing of `points`, two triangles per crossing edge with
        four cells around it) -> (vertices [cap_vertices,16] uint8, faces [cap_faces,3] int32, count [2] int32) on the device.  The vertices are
        the cloud's records (as_records), vertices[:min(count[0], cap_vertices)]; the triangles faces[:min(count[1], cap_faces)] hold vertex
        numbers, counter-clockwise seen from the side of positive tsdf (the camera's).  count holds the totals, also beyond the caps: with
        count[0] > cap_vertices or count[1] > cap_faces the mesh is incomplete (save_mesh runs again).  Caps None: default_mesh_caps().  out:
        optional (vertices, faces, count) destinations; workspace: optional int32 tensor of at least mesh_workspace_numel() elements, whose
        contents do not matter.  Four launches on the current stream, no host synchronisation."""
        min_weight = check_min_weight(min_weight)
        dv, df = self.default_mesh_caps()
        cap_vertices, cap_faces = dv if cap_vertices is None else int(cap_vertices), df if cap_faces is None else int(cap_faces)
        if not 1 <= cap_vertices <= 0x7fffffff or not 1 <= cap_faces <= 0x7fffffff:
            raise ValueError(f"TsdfVolume.mesh: cap_vertices and cap_faces must lie in [1, 2^31), got {cap_vertices}, {cap_faces}")
        vertices, faces, count = out if out is not None else (None, None, None)
        vertices = A.dst("tsdf_mesh", vertices, (cap_vertices, 16), torch.uint8, True, self.device)
        faces = A.dst("tsdf_mesh", faces, (cap_faces, 3), torch.int32, True, self.device)
        count = A.dst("tsdf_mesh", count, (2,), torch.int32, True, self.device)
        if workspace is None:
            workspace = torch.empty((self.mesh_workspace_numel(),), dtype=torch.int32, device=self.device)
        if not torch.is_tensor(workspace) or workspace.dtype != torch.int32 or workspace.device != self.device:
            got = f"{workspace.dtype} on {workspace.device}" if torch.is_tensor(workspace) else type(workspace).__name__
            raise L.SdeHipError(f"tsdf_mesh: workspace must be an int32 tensor on {self.device}, got {got}")
        nx, ny, nz = self.dims
        L.check(L.lib().sde_tsdf_mesh(L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(self.rgba), nx, ny, nz, self._origin, self.voxel, min_weight,
                                      L.ptr(workspace), workspace.numel() * 4, L.ptr(vertices), cap_vertices, L.ptr(faces), cap_faces, L.ptr(count),
                                      L.stream()), "sde_tsdf_mesh")
        return vertices, faces, count

    def render(self, K, C, size, near=None, far=None, step=None, min_weight=1, normals=True, picture=True, out=None):
        """The volume seen from a camera (sde_tsdf_render: ray casting) -> (depth [H,W] fp32, normal [H,W,3] fp32 or None, picture [H,W,4] uint8
        or None) on the device.  K [3,3] fp32 at the picture's size and C [4,4] fp32, world -> camera (rigid: the caller's responsibility), are
        CUDA tensors on the volume's device -- the pose `compose` chains goes in as it is.  size = (H, W).  The ray of every pixel is sampled at
        the z-depths near + i * step, i < n = ceil((far - near) / step); defaults: near = min_depth, far = max_depth, step = voxel.  depth is the
        z-depth of the first crossing from positive to negative tsdf between two valid samples (all eight voxels around a sample have weight >=
        min_weight), 0 where there is none; normal the unit normal in camera coordinates, towards the side the surface was seen from; picture
        the voxel colour with alpha 255 (picture=True needs a volume with colour); both zeros on a miss.  out: optional (depth, normal,
        picture) destinations (None for those not wanted).  One launch on the current stream, no host synchronisation."""
        min_weight = check_min_weight(min_weight)
        H, W, near, step, n = check_render(size, self.min_depth if near is None else near, self.max_depth if far is None else far,
                                           self.voxel if step is None else step)
        if picture and self.rgba is None:
            raise ValueError("TsdfVolume.render: picture=True needs a volume with colour (colour=True); pass picture=False")
        K = A.as_K("tsdf_render", K, 1, self.device)
        if torch.is_tensor(C) and C.dim() == 3:
            C = C[0]
        C = A.same_device_tensor("tsdf_render", "C", C, torch.float32, (4, 4), self.device).contiguous()
        depth, normal, pic = out if out is not None else (None, None, None)
        depth = A.dst("tsdf_render", depth, (H, W), torch.float32, True, self.device)
        normal = A.dst("tsdf_render", normal, (H, W, 3), torch.float32, bool(normals), self.device)
        pic = A.dst("tsdf_render", pic, (H, W, 4), torch.uint8, bool(picture), self.device)
        nx, ny, nz = self.dims
        L.check(L.lib().sde_tsdf_render(L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(self.rgba), nx, ny, nz, self._origin, self.voxel, min_weight,
                                        L.ptr(K), L.ptr(C), H, W, near, step, n, L.ptr(depth), L.ptr(normal), L.ptr(pic), L.stream()), "sde_tsdf_render")
        return depth, normal, pic

    def track(self, pred, ymap, xmap, K, C, size, schedule=None, dist_tol=None, scale_tol=None, min_count=None, damping=None, min_weight=1, near=None,
              far=None, step=None, state=None):
        """A frame's depth aligned with the volume (hip.align: sde_frame_align) -> the AlignState.  C [4,4] is the PREDICTED world -> camera pose
        (the chain of `compose`), size = (H, W) = (ymap.numel(), xmap.numel()).  In order, on the current stream, with no host synchronisation:
        the volume's depth and normals are rendered from C (near / far / step / min_weight as in `render`); the state is reset (D = I, scale = 1);
        one `frame_align` runs per entry of `schedule` (a sequence of modes: align.POSE, align.SCALE or both; None: align.DEFAULT_SCHEDULE).
        Afterwards state.D takes the frame's camera coordinates to those of the camera at C: world -> corrected camera is D^-1 C, which the
        caller forms with `compose(state.Dinv, C)`; state.scale [1] is the factor the frame's depth is multiplied by.  An empty volume (every ray
        misses) leaves D = I and scale = 1 with the status "too few": the host never looks.  dist_tol, scale_tol, min_count, damping: None takes
        align.DEFAULTS.  state: an AlignState of this size to run in (its buffers are reused); None makes one."""
        from . import align as AL
        H, W = AL.check_size(size)
        schedule = AL.DEFAULT_SCHEDULE if schedule is None else tuple(schedule)
        if not schedule:
            raise ValueError("TsdfVolume.track: schedule must name at least one iteration")
        kw = {k: AL.DEFAULTS[k] if v is None else v for k, v in (("dist_tol", dist_tol), ("scale_tol", scale_tol), ("min_count", min_count), ("damping", damping))}
        for mode in schedule:                                   # every argument error before the first launch
            AL.check_align(mode=mode, min_depth=self.min_depth, max_depth=self.max_depth, **kw)
        if state is None:
            state = AL.AlignState((H, W), self.device)
        if not isinstance(state, AL.AlignState) or (state.H, state.W) != (H, W) or state.device != self.device:
            raise ValueError(f"TsdfVolume.track: state must be an AlignState of size {(H, W)} on {self.device}")
        if torch.is_tensor(ymap) and torch.is_tensor(xmap) and (ymap.numel(), xmap.numel()) != (H, W):
            raise ValueError(f"TsdfVolume.track: size {(H, W)} does not match the maps ({ymap.numel()}, {xmap.numel()})")
        self.render(K, C, (H, W), near=near, far=far, step=step, min_weight=min_weight, normals=True, picture=False,
                    out=(state.model_depth, state.model_normal, None))
        state.reset()
        for mode in schedule:
            AL.frame_align(pred, ymap, xmap, K, state.model_depth, state.model_normal, state, mode=mode, min_depth=self.min_depth,
                           max_depth=self.max_depth, **kw)
        return state

    def save_mesh(self, path, min_weight=1, cap_vertices=None, cap_faces=None):
        """The mesh as a binary PLY (write_mesh_ply).  Synchronises.  When either cap was too small the mesh is taken once more with exactly the
        counted room: a truncated mesh, whose triangles would name missing vertices, is never written.  Returns (vertices, triangles) written."""
        vertices, faces, count = self.mesh(min_weight=min_weight, cap_vertices=cap_vertices, cap_faces=cap_faces)
        nv, nf = (int(c) for c in count.cpu())
        if nf == 0x7fffffff:
            raise L.SdeHipError("TsdfVolume.save_mesh: the volume holds 2^31 - 1 triangles or more, beyond what sde_tsdf_mesh can hand out")
        if nv > vertices.shape[0] or nf > faces.shape[0]:
            del vertices, faces
            vertices, faces, count = self.mesh(min_weight=min_weight, cap_vertices=max(nv, 1), cap_faces=max(nf, 1))
            assert (nv, nf) == tuple(int(c) for c in count.cpu())
        write_mesh_ply(path, as_records(vertices[:nv], nv), faces[:nf].cpu().numpy())
        return nv, nf

    def save_ply(self, path, min_weight=1, cap=None):
        """The surface points as a binary PLY (the cloud's writer and record).  Synchronises.  Returns (records written, crossings found); when
        the volume holds more crossings than `cap` records, the first `cap` are written and a warning says so."""
        points, count = self.points(min_weight=min_weight, cap=cap)
        return write_points_ply(path, points.cpu().numpy(), int(count.item()))


def write_points_ply(path, points, count):
    """points [cap,16] uint8 (host) and the count `points` / `points_host` reported -> the PLY file of the first min(count, cap) records."""
    from ..tools.demo import write_ply
    cap = points.shape[0]
    if count > cap:
        warnings.warn(f"TsdfVolume.save_ply: the volume holds {count} crossings, room was made for {cap}: the first {cap} are written "
                      f"(pass cap={count} for all of them)")
    n = min(count, cap)
    write_ply(path, as_records(points, n))
    return n, count


PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])               # one `property list uchar int vertex_indices` entry of a triangle: 13 bytes
assert PLY_FACE.itemsize == 13


def write_mesh_ply(path, vertices, faces):
    """vertices: a 1-D array of hip.cloud.RECORD; faces [n,3] int32 vertex numbers, all in [0, vertices.size) -> a binary little-endian PLY with
    the cloud's vertex properties and `element face n` / `property list uchar int vertex_indices`."""
    from ..tools.demo import PLY_PROPERTIES
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    if vertices.dtype != RECORD or vertices.ndim != 1:
        raise ValueError(f"write_mesh_ply: a 1-D array of hip.cloud.RECORD expected, got {vertices.dtype} {vertices.shape}")
    if faces.dtype != np.int32 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"write_mesh_ply: faces must be int32 [n,3], got {faces.dtype} {faces.shape}")
    if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= vertices.size):
        raise ValueError(f"write_mesh_ply: a triangle names a vertex outside [0, {vertices.size}): the mesh is incomplete")
    lines = (["ply", "format binary_little_endian 1.0", f"element vertex {vertices.size}"] + [f"property {t} {name}" for t, name in PLY_PROPERTIES]
             + [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"])
    body = np.zeros(faces.shape[0], PLY_FACE)
    body["n"], body["v"] = 3, faces
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
        vertices.tofile(f)
        body.tofile(f)


def read_mesh_ply(path):
    """What write_mesh_ply wrote -> (vertices as hip.cloud.RECORD, faces [n,3] int32).  It reads this module's layout, not PLY in general."""
    from ..tools.demo import PLY_PROPERTIES
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    want = ["ply", "format binary_little_endian 1.0", None] + [f"property {t} {name}" for t, name in PLY_PROPERTIES] + [
        None, "property list uchar int vertex_indices", "end_header", ""]
    if len(lines) != len(want) or any(w is not None and w != g for w, g in zip(want, lines)):
        raise ValueError(f"read_mesh_ply: {path} does not have the header write_mesh_ply writes")
    nv, nf = int(lines[2].removeprefix("element vertex ")), int(lines[len(PLY_PROPERTIES) + 3].removeprefix("element face "))
    if len(raw) != end + nv * RECORD.itemsize + nf * PLY_FACE.itemsize:
        raise ValueError(f"read_mesh_ply: {path} holds {len(raw) - end} bytes behind its header, {nv} vertices and {nf} triangles need "
                         f"{nv * RECORD.itemsize + nf * PLY_FACE.itemsize}")
    vertices = np.frombuffer(raw, RECORD, nv, end).copy()
    body = np.frombuffer(raw, PLY_FACE, nf, end + nv * RECORD.itemsize)
    if nf and not bool((body["n"] == 3).all()):
        raise ValueError(f"read_mesh_ply: {path} holds a face that is no triangle")
    return vertices, np.ascontiguousarray(body["v"], dtype=np.int32).reshape(nf, 3)


# ---- host twins ---------------------------------------------------------------------------------------------------------------------------------
def compose_host(T, C):
    """The host twin of sde_pose_compose: T, C [4,4] float32 -> the new C (T C with the documented order of operations)."""
    f32 = np.float32
    T, C = np.asarray(T, dtype=f32).reshape(4, 4), np.asarray(C, dtype=f32).reshape(4, 4)
    out = np.zeros((4, 4), f32)
    out[3, 3] = 1
    with np.errstate(all="ignore"):
        for r in range(3):
            row = T[r, 0] * C[0] + T[r, 1] * C[1] + T[r, 2] * C[2]
            row[3] = row[3] + T[r, 3]
            out[r] = row
    return out


def centres_np(n, o, voxel):
    """The centres of n voxels along one axis: o + ((float)i + 0.5f) * voxel, float32."""
    f32 = np.float32
    return f32(o) + (np.arange(n, dtype=f32) + f32(0.5)) * f32(voxel)


def integrate_host(tsdf, weight, rgba, pred, ymap, xmap, K, C, frame, origin, voxel, trunc, max_weight, min_depth, max_depth):
    """The host twin of sde_tsdf_integrate.  tsdf, weight [nz,ny,nx] float32 and rgba [nz,ny,nx,4] uint8 (or None) are updated IN PLACE with
    the bits the kernel writes; pred [ph,pw] float32, ymap [H] / xmap [W] int, K [3,3], C [4,4], frame [H,W,3] uint8 or None.  Returns the
    bool [nz,ny,nx] mask of the voxels that were kept (the others are untouched)."""
    f32 = np.float32
    nz, ny, nx = tsdf.shape
    pred, ymap, xmap = np.asarray(pred, dtype=f32), np.asarray(ymap), np.asarray(xmap)
    H, W = ymap.size, xmap.size
    voxel, trunc, max_weight, lo, hi = f32(voxel), f32(trunc), f32(max_weight), f32(min_depth), f32(max_depth)
    wx = centres_np(nx, origin[0], voxel)[None, None, :]
    wy = centres_np(ny, origin[1], voxel)[None, :, None]
    wz = centres_np(nz, origin[2], voxel)[:, None, None]
    with np.errstate(all="ignore"):
        _, _, qz, X, Y = pinhole_move_project_np(K, C, wx, wy, wz)
        keep = (qz > 0) & (qz < np.inf)
        ok, ix, iy = nearest_pixel_np(X, Y)
        keep = keep & ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        ix, iy = np.where(keep, ix, 0), np.where(keep, iy, 0)
        my, mx = ymap[iy], xmap[ix]
        keep &= (my >= 0) & (mx >= 0)
        d = pred[np.where(keep, my, 0), np.where(keep, mx, 0)]
        keep &= np.isfinite(d) & (lo < d) & (d <= hi)
        sdf = d - qz
        keep &= sdf >= -trunc
        t = np.fmin(f32(1), sdf / trunc)
        w0, t0 = weight[keep], tsdf[keep]
        w1 = w0 + f32(1)
        tsdf[keep] = (t0 * w0 + t[keep]) / w1
        weight[keep] = np.fmin(w1, max_weight)
        if frame is not None and rgba is not None:
            sel = keep & (sdf <= trunc)
            w0, w1 = w0[sel[keep]], w1[sel[keep]]
            f = np.asarray(frame)[iy[sel], ix[sel]].astype(f32)                                  # [n,3]
            c = (rgba[sel][:, :3].astype(f32) * w0[:, None] + f) / w1[:, None]
            new = np.full((c.shape[0], 4), 255, np.uint8)
            new[:, :3] = (c + f32(0.5)).astype(np.uint8)
            rgba[sel] = new
    return keep


def crossings_np(tsdf, weight, min_weight):
    """bool [nz,ny,nx,3]: voxel v and its +1 neighbour along x, y, z are both valid and differ in (tsdf < 0)."""
    nz, ny, nx = tsdf.shape
    valid, neg = weight >= np.float32(check_min_weight(min_weight)), tsdf < 0
    cross = np.zeros((nz, ny, nx, 3), bool)
    cross[:, :, :-1, 0] = valid[:, :, :-1] & valid[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    cross[:, :-1, :, 1] = valid[:, :-1] & valid[:, 1:] & (neg[:, :-1] != neg[:, 1:])
    cross[:-1, :, :, 2] = valid[:-1] & valid[1:] & (neg[:-1] != neg[1:])
    return cross


def points_host(tsdf, weight, rgba, origin, voxel, min_weight=1, cap=None):
    """The host twin of sde_tsdf_points -> (records, count): the structured array (hip.cloud.RECORD) of the first min(count, cap) crossings in
    the kernel's order (ascending voxel, then axis) with the bits it writes, and the total number of crossings."""
    f32 = np.float32
    tsdf, weight = np.asarray(tsdf, dtype=f32), np.asarray(weight, dtype=f32)
    nz, ny, nx = tsdf.shape
    voxel = f32(voxel)
    cross = crossings_np(tsdf, weight, min_weight)
    k, j, i, a = np.nonzero(cross)                                # C order: ascending voxel, then axis
    count = int(k.size)
    if cap is not None:
        k, j, i, a = (x[:int(cap)] for x in (k, j, i, a))
    kn, jn, in_ = k + (a == 2), j + (a == 1), i + (a == 0)
    rec = np.zeros(k.size, RECORD)
    with np.errstate(all="ignore"):
        tv, tn = tsdf[k, j, i], tsdf[kn, jn, in_]
        f = tv / (tv - tn)
        along = f * voxel
        cx, cy, cz = centres_np(nx, origin[0], voxel)[i], centres_np(ny, origin[1], voxel)[j], centres_np(nz, origin[2], voxel)[k]
        rec["x"], rec["y"], rec["z"] = np.where(a == 0, cx + along, cx), np.where(a == 1, cy + along, cy), np.where(a == 2, cz + along, cz)
        rec["alpha"] = 255
        if rgba is not None:
            own = f < f32(0.5)
            col = np.asarray(rgba)[np.where(own, k, kn), np.where(own, j, jn), np.where(own, i, in_)]
            rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    return rec, count


# the 12 edges of a cell in the order of include/sde_hip.h: (axis, corner offset (di, dj, dk) the edge starts at)
CELL_EDGES = tuple((a, tuple(np.insert((db, dc), a, 0))) for a in range(3) for db, dc in ((0, 0), (1, 0), (0, 1), (1, 1)))


def mesh_host(tsdf, weight, rgba, origin, voxel, min_weight=1, cap_vertices=None, cap_faces=None):
    """The host twin of sde_tsdf_mesh -> (vertices, faces, count): the structured array (hip.cloud.RECORD) of the first min(count[0],
    cap_vertices) vertices in ascending cell index, the first min(count[1], cap_faces) triangles as int32 [n,3] (ascending voxel, then axis, the
    two triangles of a quad next to each other; vertex numbers are the true ones, also beyond cap_vertices) and count = int32 [vertices,
    triangles], the totals: the bits the kernels write."""
    f32 = np.float32
    tsdf, weight = np.asarray(tsdf, dtype=f32), np.asarray(weight, dtype=f32)
    nz, ny, nx = tsdf.shape
    voxel = f32(voxel)
    cross = crossings_np(tsdf, weight, min_weight)
    cz, cy, cx = max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)                              # cells along each axis
    edge = lambda a, d: cross[d[2]:d[2] + cz, d[1]:d[1] + cy, d[0]:d[0] + cx, a]             # that edge of every cell
    has = np.zeros((cz, cy, cx), bool)
    for a, d in CELL_EDGES:
        has |= edge(a, d)
    k, j, i = np.nonzero(has)                                     # C order: ascending cell index
    nv = int(k.size)
    number = np.full((nz, ny, nx), -1, np.int32)                  # cell -> vertex number
    number[k, j, i] = np.arange(nv, dtype=np.int32)
    if cap_vertices is not None:
        k, j, i = (x[:int(cap_vertices)] for x in (k, j, i))
    rec = np.zeros(k.size, RECORD)
    cen = [centres_np(n, o, voxel) for n, o in zip((nx, ny, nz), origin)]
    s = [np.zeros(k.size, f32) for _ in range(3)]
    col = np.zeros((k.size, 3), np.int64)
    m = np.zeros(k.size, np.int64)
    with np.errstate(all="ignore"):
        for a, d in CELL_EDGES:
            lo = (i + d[0], j + d[1], k + d[2])
            hi = tuple(lo[b] + (a == b) for b in range(3))
            on = cross[lo[2], lo[1], lo[0], a]
            tv, tn = tsdf[lo[2], lo[1], lo[0]], tsdf[hi[2], hi[1], hi[0]]
            f = tv / (tv - tn)
            along = f * voxel
            for b in range(3):
                c = cen[b][lo[b]]
                s[b] = np.where(on, s[b] + (c + along if a == b else c), s[b])
            if rgba is not None:
                own = f < f32(0.5)
                pick = [np.where(own, lo[b], hi[b]) for b in range(3)]
                col += np.where(on[:, None], np.asarray(rgba)[pick[2], pick[1], pick[0], :3].astype(np.int64), 0)
            m += on
        fm = m.astype(f32)
        rec["x"], rec["y"], rec["z"] = s[0] / fm, s[1] / fm, s[2] / fm
        byte = (col.astype(f32) / fm[:, None] + f32(0.5)).astype(np.uint8)
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = byte[:, 0], byte[:, 1], byte[:, 2], 255

    k, j, i, a = np.nonzero(cross)                                # C order: ascending voxel, then axis
    inner = [(1 <= x) & (x <= n - 2) for x, n in zip((i, j, k), (nx, ny, nz))]
    sel = np.where(a == 0, inner[1] & inner[2], np.where(a == 1, inner[0] & inner[2], inner[0] & inner[1]))
    k, j, i, a = (x[sel] for x in (k, j, i, a))
    nq = int(k.size)
    nf = min(2 * nq, 0x7fffffff)
    if cap_faces is not None:
        k, j, i, a = (x[:(int(cap_faces) + 1) // 2] for x in (k, j, i, a))
    b, c = np.where(a == 0, 1, 0), np.where(a == 2, 1, 2)         # b < c, the other two axes
    pos = np.stack([i, j, k], 1)
    rows = np.arange(k.size)

    def q(db, dc):
        p = pos.copy()
        p[rows, b] += db
        p[rows, c] += dc
        return number[p[:, 2], p[:, 1], p[:, 0]]
    q0, q1, q2, q3 = q(-1, -1), q(0, -1), q(0, 0), q(-1, 0)
    keep = (tsdf[k, j, i] < 0) != (a == 1)
    p1, p3 = np.where(keep, q1, q3), np.where(keep, q3, q1)
    faces = np.stack([q0, p1, q2, q0, q2, p3], 1).astype(np.int32).reshape(-1, 3)
    if cap_faces is not None:
        faces = faces[:int(cap_faces)]
    return rec, np.ascontiguousarray(faces), np.array([nv, nf], np.int32)


def render_host(tsdf, weight, rgba, K, C, size, origin, voxel, near, step, n, min_weight=1):
    """The host twin of sde_tsdf_render -> (depth [H,W] float32, normal [H,W,3] float32, picture [H,W,4] uint8 or None without rgba): the bits the
    kernel writes.  The same fp32 operations in the same order, vectorised over the pixels with a loop over the n samples: the FULL march, no
    sample is skipped."""
    f32 = np.float32
    tsdf, weight = np.asarray(tsdf, dtype=f32), np.asarray(weight, dtype=f32)
    nz, ny, nx = tsdf.shape
    H, W = (int(s) for s in size)
    K, C = np.asarray(K, dtype=f32).reshape(3, 3), np.asarray(C, dtype=f32).reshape(4, 4)
    R, t = C[:3, :3], C[:3, 3]
    voxel, near, step, min_weight = f32(voxel), f32(near), f32(step), f32(check_min_weight(min_weight))
    o = [f32(x) for x in origin]
    depth, normal = np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    picture = np.zeros((H, W, 4), np.uint8) if rgba is not None else None
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    if not (np.isfinite(C[:3]).all() and np.isfinite([fx, cx, fy, cy]).all()) or min(nx, ny, nz) < 2:
        return depth, normal, picture
    flat_t, flat_w = tsdf.reshape(-1), weight.reshape(-1)
    flat_c = np.asarray(rgba).reshape(-1, 4) if rgba is not None else None
    sy, sz = nx, nx * ny
    corner = [(c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz for c in range(8)]
    with np.errstate(all="ignore"):
        k00, k11, k02, k12 = f32(1) / fx, f32(1) / fy, (f32(-1) * cx) / fx, (f32(-1) * cy) / fy
        rx = np.broadcast_to((k00 * np.arange(W, dtype=f32) + k02)[None, :], (H, W)).reshape(-1)
        ry = np.broadcast_to((k11 * np.arange(H, dtype=f32) + k12)[:, None], (H, W)).reshape(-1)
        P = rx.size
        live = np.ones(P, bool)                                  # no hit so far
        prev = np.zeros(P, bool)
        tp = np.zeros(P, f32)
        dep, nor, pic = depth.reshape(-1), normal.reshape(-1, 3), (picture.reshape(-1, 4) if picture is not None else None)
        top = [f32(nx - 2), f32(ny - 2), f32(nz - 2)]
        for i in range(int(n)):
            if not live.any():
                break
            s = near + f32(i) * step
            d = [s * rx - t[0], s * ry - t[1], np.full(P, s - t[2], f32)]
            g, b = [], []
            valid = live.copy()
            for r in range(3):
                w = R[0, r] * d[0] + R[1, r] * d[1] + R[2, r] * d[2]
                gr = (w - o[r]) / voxel - f32(0.5)
                br = np.floor(gr)
                valid &= np.isfinite(gr) & (br >= 0) & (br <= top[r])
                g.append(gr)
                b.append(br)
            at = np.nonzero(valid)[0]
            bi = [b[r][at].astype(np.int64) for r in range(3)]
            base = bi[2] * sz + bi[1] * sy + bi[0]
            ok = np.ones(at.size, bool)
            for c in corner:
                ok &= flat_w[base + c] >= min_weight
            prev[live & ~valid] = False                          # outside the grid ...
            prev[at[~ok]] = False                                # ... or next to a voxel that is not valid: the sample clears prev
            at, base = at[ok], base[ok]
            f = [g[r][at] - b[r][at] for r in range(3)]
            T = [flat_t[base + c] for c in corner]
            cz = [T[2 * q] + f[0] * (T[2 * q + 1] - T[2 * q]) for q in range(4)]
            e = [cz[0] + f[1] * (cz[1] - cz[0]), cz[2] + f[1] * (cz[3] - cz[2])]
            ti = e[0] + f[2] * (e[1] - e[0])
            hit = prev[at] & (tp[at] > 0) & (ti <= 0)
            ha = at[hit]
            if ha.size:
                sp = near + f32(i - 1) * step
                th, tq = ti[hit], tp[ha]
                dep[ha] = sp + step * (tq / (tq - th))
                fh = [x[hit] for x in f]
                X = [(T[2 * q + 1] - T[2 * q])[hit] for q in range(4)]
                x0, x1 = X[0] + fh[1] * (X[1] - X[0]), X[2] + fh[1] * (X[3] - X[2])
                gx = x0 + fh[2] * (x1 - x0)
                y0, y1 = (cz[1] - cz[0])[hit], (cz[3] - cz[2])[hit]
                gy = y0 + fh[2] * (y1 - y0)
                gz = (e[1] - e[0])[hit]
                ln = np.sqrt(gx * gx + gy * gy + gz * gz)
                unit = (ln > 0) & (ln < np.inf)
                for r in range(3):
                    nor[ha, r] = np.where(unit, (R[r, 0] * gx + R[r, 1] * gy + R[r, 2] * gz) / ln, f32(0))
                if pic is not None:
                    near_c = base[hit] + (fh[0] >= f32(0.5)) * 1 + (fh[1] >= f32(0.5)) * sy + (fh[2] >= f32(0.5)) * sz
                    pic[ha, :3] = flat_c[near_c, :3]
                    pic[ha, 3] = 255
                live[ha] = False
            keep = at[~hit]
            prev[keep] = True
            tp[keep] = ti[~hit]
    return depth, normal, picture

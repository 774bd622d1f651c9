"""File loading steps (reference: detectron2/data/preprocess/loading.py:L25-123 LoadImg, LoadDepth, LoadMask, LoadLidar).

The reference decodes with OpenCV (absent here); Pillow decodes the same PNG bytes: an 8-bit RGB PNG gives the array cv2.imread +
COLOR_BGR2RGB gives, a 16-bit grayscale PNG the array cv2.imread(path, -1) gives (PNG decoding is lossless, so the arrays are equal by the
format's definition; tests write PNGs and read them back).  Waymo frames are JPEGs: read_rgb decodes them with Pillow's libjpeg, and JPEG
decoding is NOT bit-exact across decoders (IDCT and chroma up-sampling differ), so parity with cv2's decoder is unpinned -- the test pins
only that LoadImg returns the array Pillow decodes."""
import os

import numpy as np

from .build import PREPROCESS_REGISTRY, Preprocess


def read_rgb(path):
    from PIL import Image
    if not os.path.isfile(path):
        raise AssertionError(f"'{path} does not exist!'")       # the reference asserts on cv2.imread's None
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8).copy()


def read_depth_png(path):
    """KITTI depth maps are 16-bit PNGs of depth * 256; the reference divides by 255 (sic, loading.py:L59) -- kept."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im)
    if arr.dtype not in (np.uint16, np.int32, np.uint8):
        arr = arr.astype(np.int32)
    return arr.astype(np.float32) / 255


def read_mask_png(path):
    """Segmentation masks are 8- or 16-bit single-channel PNGs; the integers as float32: cv2.imread(path, -1).astype(np.float32)."""
    from PIL import Image
    if not os.path.isfile(path):
        raise AssertionError(f"'{path} does not exist!'")       # the reference's text (its assert comes after cv2.imread's None has already failed)
    with Image.open(path) as im:
        arr = np.asarray(im)
    if arr.dtype == bool:                                       # 1-bit PNGs decode to bool with Pillow, to 0 / 255 with cv2
        arr = arr.astype(np.uint8) * 255
    return arr.astype(np.float32)


@PREPROCESS_REGISTRY.register()
class LoadImg(Preprocess):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.load_ctx = cfg.get("WITH_CTX", False)

    def forward(self, data_dict):
        data_dict["img"] = read_rgb(data_dict["metadata"]["img_dir"])
        if self.load_ctx:
            data_dict["ctx_img"] = [read_rgb(p) for p in data_dict["metadata"]["ctx_img_dir"]]
        return data_dict


@PREPROCESS_REGISTRY.register()
class LoadDepth(Preprocess):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.load_ctx = cfg.get("WITH_CTX", False)
        self.keep_orig_for_eval = cfg.get("KEEP_ORIG", False)

    @staticmethod
    def _load(depth_dir):
        ext = os.path.splitext(depth_dir)[-1]
        if ext == ".npz":
            return np.load(depth_dir)["velodyne_depth"].astype(np.float32)
        if ext == ".png":
            return read_depth_png(depth_dir)
        raise NotImplementedError(depth_dir)

    def forward(self, data_dict):
        data_dict["depth"] = self._load(data_dict["metadata"]["depth_dir"])
        if self.keep_orig_for_eval:
            data_dict["depth_orig"] = data_dict["depth"].copy()
        if self.load_ctx:
            data_dict["ctx_depth"] = [self._load(p) for p in data_dict["metadata"]["ctx_depth_dir"]]
        return data_dict


@PREPROCESS_REGISTRY.register()
class LoadMask(Preprocess):
    """`mask` and `ctx_mask` (always both: loading.py:L88-96 has no WITH_CTX switch) from metadata['mask_dir'] / ['ctx_mask_dir']."""

    def forward(self, data_dict):
        data_dict["mask"] = read_mask_png(data_dict["metadata"]["mask_dir"])
        data_dict["ctx_mask"] = [read_mask_png(p) for p in data_dict["metadata"]["ctx_mask_dir"]]
        return data_dict


@PREPROCESS_REGISTRY.register()
class LoadLidar(Preprocess):
    """Velodyne scans: a flat float32 .bin read as [-1, LOAD_DIM], of which USE_DIM keeps the leading columns (int) or the listed ones."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.load_ctx = cfg.get("WITH_CTX", False)
        self.load_dim = cfg.get("LOAD_DIM", 4)
        self.use_dim = cfg.get("USE_DIM", 3)

    def _load(self, lidar_dir):
        if os.path.splitext(lidar_dir)[-1] != ".bin":
            raise NotImplementedError(lidar_dir)
        scan = np.fromfile(lidar_dir, dtype=np.float32).reshape(-1, self.load_dim)
        return scan[:, :self.use_dim] if isinstance(self.use_dim, int) else scan[:, list(self.use_dim)]

    def forward(self, data_dict):
        data_dict["lidar"] = self._load(data_dict["metadata"]["lidar_dir"])
        if self.load_ctx:
            data_dict["ctx_lidar"] = [self._load(p) for p in data_dict["metadata"]["ctx_lidar_dir"]]
        return data_dict


LIDAR_RAW = ("lidar_points", "lidar_count", "lidar_window", "lidar_clip", "lidar_flags", "lidar_proj", "lidar_window_orig")


@PREPROCESS_REGISTRY.register()
class LidarDepth(Preprocess):
    """Depth ground truth projected from the raw scan (an addition of this package; the routine is generate_depth_map of monodepth2 / packnet-sfm,
    stated in include/sde_hip.h).  Stands where LoadDepth stands, behind LoadLidar and LoadImg; needs `lidar`, `lidar_proj` (KittiDepthV2 with
    DEPTH_TYPE: "lidar") and `img`.

    Host mode: `depth` [H,W] float32 at the image's size from hip.lidar.lidar_depth_np (`depth_orig` with KEEP_ORIG); `lidar` and `lidar_proj` are
    removed, every later step works as behind LoadDepth.
    ON_DEVICE: True: nothing is projected here.  The step emits `lidar_points` [MAX_POINTS,3] float32 (zero-padded; pre-filtered to x >= 0 with
    FRONT_ONLY, which is what the kernel would drop), `lidar_count`, `lidar_window` int32 [x0, y0, w, h] (the whole image), `lidar_clip` (0: none),
    `lidar_flags`; KBCrop / CropTopTo / RandomCrop move and shrink the window, ClipDepth records its MAX_DEPTH, and data/device_aug.py projects
    straight into the final window on the GPU (sde_lidar_depth).  KEEP_ORIG keeps the whole-image window as `lidar_window_orig`.  The capacity is
    fixed so that batches stack and the prefetcher's persistent buffers never change shape; a scan with more points raises."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.vel_depth = bool(cfg.get("VEL_DEPTH", False))
        self.front_only = bool(cfg.get("FRONT_ONLY", True))
        self.keep_orig_for_eval = cfg.get("KEEP_ORIG", False)
        self.on_device = bool(cfg.get("ON_DEVICE", False))
        self.max_points = int(cfg.get("MAX_POINTS", 131072))

    def forward(self, data_dict):
        from ...hip.lidar import flag_bits, lidar_depth_np
        scan = np.asarray(data_dict.pop("lidar"), dtype=np.float32)[:, :3]
        H, W = data_dict["img"].shape[:2]
        if not self.on_device:
            data_dict["depth"] = lidar_depth_np(scan, data_dict.pop("lidar_proj"), (0, 0), H, W, self.vel_depth, self.front_only)
            if self.keep_orig_for_eval:
                data_dict["depth_orig"] = data_dict["depth"].copy()
            return data_dict
        if self.front_only:
            scan = scan[scan[:, 0] >= 0]
        if len(scan) > self.max_points:
            raise ValueError(f"LidarDepth: the scan {data_dict['metadata'].get('lidar_dir', '')} has {len(scan)} points, MAX_POINTS is {self.max_points}: raise MAX_POINTS")
        points = np.zeros((self.max_points, 3), dtype=np.float32)
        points[:len(scan)] = scan
        data_dict["lidar_points"] = points
        data_dict["lidar_count"] = np.int32(len(scan))
        data_dict["lidar_window"] = np.array([0, 0, W, H], dtype=np.int32)
        data_dict["lidar_clip"] = np.float32(0)
        data_dict["lidar_flags"] = np.int32(flag_bits(self.vel_depth, self.front_only))
        data_dict["lidar_proj"] = np.ascontiguousarray(data_dict["lidar_proj"], dtype=np.float32)
        if self.keep_orig_for_eval:
            data_dict["lidar_window_orig"] = data_dict["lidar_window"].copy()
        return data_dict

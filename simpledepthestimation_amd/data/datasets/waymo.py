"""Waymo Open Dataset reader (reference: detectron2/data/datasets/waymo.py:L15-155 ``WaymoDepth``).

On-disk formats (written by the reference's tools/extract_waymo_data.py): the split file is a pickle
``{segment: {"cams": {cam: {"intrinsics", "extrinsics"}}, "frames": {frame_time: {"cams": {cam: cam_timestamp}}}}}``; images are
``<DATA_ROOT>/<segment>/<cam>/<cam_timestamp>.jpg``, projected lidar depth ``<DEPTH_ROOT>/.../<cam_timestamp>.png`` (16-bit) and, with MASK_ROOT,
segmentation masks ``<MASK_ROOT>/.../<cam_timestamp>.png``.  Inside a segment the frames are sorted by frame_time and thinned with
``[::DOWNSAMPLE]``; segments keep the pickle's order.  With FORWARD_CONTEXT / BACKWARD_CONTEXT a sample survives only if its neighbours at
+-STRIDE positions of the thinned list lie in the same segment.  ``__getitem__`` returns a LIST, one preprocessed dict per camera of
USE_CAMS; ``batch_collator`` folds the camera dimension into the batch.  No file is opened before the preprocess chain runs.

Two deliberate deviations from the reference:
  * USE_CAMS given as a bare string names ONE camera (the reference iterates the string's characters, so its own default 'FRONT' looks up the
    cameras 'F', 'R', 'O', ...); lists and tuples are taken as they are;
  * contexts with STRIDE 0 raise a ValueError naming the key (the reference fails inside range() with "arg 3 must not be zero")."""
import logging
import os
import pickle

import numpy as np

from ..build import DATASET_REGISTRY, DatasetBase, collate_samples

logger = logging.getLogger(__name__)


@DATASET_REGISTRY.register()
class WaymoDepth(DatasetBase):
    def __init__(self, dataset_cfg, cfg):
        super().__init__(dataset_cfg, cfg)
        self.data_root, self.depth_root, self.split_file = dataset_cfg.DATA_ROOT, dataset_cfg.get("DEPTH_ROOT", ""), dataset_cfg.SPLIT
        self.mask_root = dataset_cfg.get("MASK_ROOT", None)
        self.downsample = dataset_cfg.get("DOWNSAMPLE", 1)
        use_cams = dataset_cfg.get("USE_CAMS", "FRONT")
        self.use_cams = [use_cams] if isinstance(use_cams, str) else list(use_cams)
        self.with_depth = dataset_cfg.get("WITH_DEPTH", False)
        self.with_mask = self.mask_root is not None
        self.forward_context = dataset_cfg.get("FORWARD_CONTEXT", 0)
        self.backward_context = dataset_cfg.get("BACKWARD_CONTEXT", 0)
        self.stride = dataset_cfg.get("STRIDE", 0)
        self.with_pose = dataset_cfg.get("WITH_POSE", False)
        self.with_context_depth = dataset_cfg.get("WITH_CONTEXT_DEPTH", False)

        with open(self.split_file, "rb") as f:
            infos = pickle.load(f)
        self.metadatas, self.calib_cache = [], {}
        for segment, seg_info in infos.items():
            frames = [(segment, frame, frame_info["cams"]) for frame, frame_info in seg_info["frames"].items()]
            self.metadatas.extend(sorted(frames, key=lambda m: m[1])[::self.downsample])
            self.calib_cache[segment] = seg_info["cams"]
        if self.downsample > 1:
            logger.info("Downsample dataset to 1/%d!", self.downsample)
        logger.info("Loaded %d samples", len(self.metadatas))

        self.context_list = [[] for _ in self.metadatas]
        self.with_context = self.backward_context != 0 or self.forward_context != 0
        if self.with_context:
            if self.stride == 0:
                raise ValueError("DATASETS.*.STRIDE must not be 0 when FORWARD_CONTEXT / BACKWARD_CONTEXT ask for context frames")
            self.valid_inds = []
            for idx, (segment, _, _) in enumerate(self.metadatas):
                for offset in range(-self.backward_context * self.stride, self.forward_context * self.stride + 1, self.stride):
                    j = idx + offset
                    if offset != 0 and 0 <= j < len(self.metadatas) and self.metadatas[j][0] == segment:
                        self.context_list[idx].append(j)
                if len(self.context_list[idx]) == self.backward_context + self.forward_context:
                    self.valid_inds.append(idx)
        else:
            self.valid_inds = list(range(len(self.metadatas)))
        logger.info("After context filtering, %d samples left", len(self.valid_inds))
        if not self.metadatas:
            logger.warning("Empty dataset!")

    def __len__(self):
        return len(self.valid_inds)

    def __getitem__(self, idx_):
        idx = self.valid_inds[idx_]
        segment, frame_time, img_time = self.metadatas[idx]
        ctx = [self.metadatas[j] for j in self.context_list[idx]]
        data_allcams = []
        for cam in self.use_cams:
            data = {"metadata": {"segment": segment, "frame_time": frame_time, "cam": cam, "use_cams": self.use_cams, "img_time": img_time,
                                 "img_dir": self._get_img_dir(segment, img_time[cam], cam), "depth_dir": self._get_depth_dir(segment, img_time[cam], cam),
                                 "ctx_img_dir": [self._get_img_dir(m[0], m[2][cam], cam) for m in ctx],
                                 "ctx_depth_dir": [self._get_depth_dir(m[0], m[2][cam], cam) for m in ctx]},
                    "intrinsics": self.calib_cache[segment][cam]["intrinsics"][:3, :3].astype(np.float32)}
            if self.with_mask:
                data["metadata"]["mask_dir"] = self._get_mask_dir(segment, img_time[cam], cam)
                data["metadata"]["ctx_mask_dir"] = [self._get_mask_dir(m[0], m[2][cam], cam) for m in ctx]
            data_allcams.append(self.preprocess(data))
        return data_allcams

    def _get_img_dir(self, segment, img_time, cam):
        return os.path.join(self.data_root, segment, cam, f"{img_time}.jpg")

    def _get_depth_dir(self, segment, img_time, cam):
        return os.path.join(self.depth_root, segment, cam, f"{img_time}.png")

    def _get_mask_dir(self, segment, img_time, cam):
        return os.path.join(self.mask_root, segment, cam, f"{img_time}.png")

    def batch_collator(self, batch_list):
        """list (samples) of lists (cameras) of dicts -> the batch dict: the camera dimension is absorbed into the batch (sample-major), `mask` joins
        `depth` as a [B,1,H,W] tensor, `ctx_mask` joins `ctx_depth` as a list of [B,1,H,W] arrays; the rest as KittiDepthV2's, ON_DEVICE entries included."""
        return collate_samples([d for cams in batch_list for d in cams], maps=("depth", "mask"), map_lists=("ctx_depth", "ctx_mask"))

"""Default config values of the keys on the path (reference: detectron2/config/defaults.py).

COMPUTE_DTYPE is new: "fp32" reproduces the reference numerics (parity mode), "bf16" stores activations/weights of the
convolutions in bf16 with fp32 accumulation, statistics and losses (BASELINE.json config 2).
"""
from .config import CfgNode as CN

_C = CN()
_C.VERSION = 2
_C.MODEL = CN()
_C.MODEL.META_ARCHITECTURE = "SupDepthModel"
_C.MODEL.DEVICE = "cuda"
_C.MODEL.WEIGHTS = ""
_C.MODEL.MAX_DEPTH = 80
_C.MODEL.PIXEL_MEAN = [0.485, 0.456, 0.406]
_C.MODEL.PIXEL_STD = [0.229, 0.224, 0.225]
_C.MODEL.COMPUTE_DTYPE = "fp32"
_C.MODEL.DATASET = ""                      # BtsModel: "kitti" scales the final depth by focal / 715.0873
_C.MODEL.DEPTH_NET = CN()
_C.MODEL.DEPTH_NET.NAME = "DepthResNet"
_C.MODEL.DEPTH_NET.ENCODER_NAME = "18"
_C.MODEL.DEPTH_NET.UPSAMPLE_DEPTH = False
_C.MODEL.DEPTH_NET.VERSION = "1A"          # PackNet01 only (packnet_1a.yaml)
# --- BtsModel only (projects/Supervised/configs/bts_r50.yaml; BTSNet.py:L337-413) ---
_C.MODEL.DEPTH_NET.BTS_SIZE = 512          # decoder width (num_features)
_C.MODEL.DEPTH_NET.BN_NO_TRACK = False     # bn_init_as_tf: m.eval() at build time, undone by the training loop's model.train()
_C.MODEL.DEPTH_NET.FIX_1ST_CONV = False    # also freeze layer1.0 of the encoder
_C.MODEL.DEPTH_NET.FIX_1ST_CONVS = False   # also freeze layer1.0 and layer1.1
# --- GoogleResNet only (projects/MotionLearning/configs/resnet18.yaml; GoogleResNet.py:L126-155) ---
_C.MODEL.DEPTH_NET.NORM = "randLN"         # encoder norm layer: "randLN" (RandLayerNorm), "BN" or None (BN)
_C.MODEL.DEPTH_NET.NOISE_STDDEV = 0.5      # RandLayerNorm noise reached at the end of the ramp
_C.MODEL.DEPTH_NET.RAMPUP_ITERS = 0        # > 0: the noise ramps as NOISE_STDDEV * min(step / RAMPUP_ITERS, 1)^2 (0: the modules keep stddev 0.5)
_C.MODEL.DEPTH_NET.LEARN_SCALE = False     # adds decoder.scale (ones(1)), which the forward pass never reads
_C.MODEL.POSE_NET = CN()
_C.MODEL.POSE_NET.NAME = "PoseNet"
_C.MODEL.POSE_NET.NUM_CONTEXTS = 2
# GooglePoseNet / GoogleMotionNet (projects/MotionLearning/configs/Base.yaml); PoseNet reads none of these
_C.MODEL.POSE_NET.USE_DEPTH = True           # pose_net_input carries 2 x (RGB + depth) = 8 channels (False: 6)
_C.MODEL.POSE_NET.GROUP_NORM = False         # GroupNorm(16) between every convolution and its ReLU (never in refiner0)
_C.MODEL.POSE_NET.MASK_MOTION = True         # keep the motion field only where its norm exceeds the batch mean
_C.MODEL.POSE_NET.LEARN_SCALE = True         # rot_scale / trans_scale parameters (False: the constant 0.01)
_C.MODEL.POSE_NET.SCALE_CONSTRAIN = "clip"   # "clip", "clip_ste" or "softplus" (GoogleMotionNet; anything else raises NotImplementedError)
_C.MODEL.POSE_NET.BURN_IN_ITERS = 20000      # > 0: engine/loops.py ramps motion_weight as clip(2 * step / BURN_IN_ITERS - 1, 0, 1) before every step
_C.LOSS = CN()
_C.LOSS.SSIM_WEIGHT = 0.85
_C.LOSS.C1 = 1e-4
_C.LOSS.C2 = 9e-4
_C.LOSS.CLIP = 0.0
_C.LOSS.AUTOMASK = True
_C.LOSS.SMOOTHNESS_WEIGHT = 1e-3
_C.LOSS.PHOTOMETRIC_REDUCE = "min"
_C.LOSS.SUPERVISED_WEIGHT = 0.0
_C.LOSS.VARIANCE_FOCUS = 0.85
_C.LOSS.VAR_LOSS_WEIGHT = 0.0
_C.SOLVER = CN()
# --- values of detectron2/config/defaults.py:L101-131 for the keys the reference defines (merging one of its YAMLs here gives what merging it there gives) ---
_C.SOLVER.IMS_PER_BATCH = 16
_C.SOLVER.DEPTH_LR = 1e-3
_C.SOLVER.MAX_EPOCHS = 10
_C.SOLVER.CHECKPOINT_PERIOD = 1
_C.SOLVER.REFERENCE_WORLD_SIZE = 0
# --- keys the reference's defaults do not define (its project YAMLs add them through set_new_allowed, utils/setup.py:L18): neutral values ---
_C.SOLVER.POSE_LR = 1e-3
_C.SOLVER.DEPTH_END_LR = 1e-5
_C.SOLVER.LR_STEPS = ()
_C.SOLVER.GAMMA = 0.1
_C.SOLVER.CLIP_GRAD = 0                    # MotionLearning (its Base.yaml: 10): max total gradient norm of nn.utils.clip_grad_norm_; 0: no clipping
_C.SOLVER.AMP = False                      # fp16 storage + dynamic loss scaling (engine/train_loop.py:L294-341 AMPTrainer); needs MODEL.COMPUTE_DTYPE fp16
_C.TEST = CN()
_C.TEST.EVAL_PERIOD = 1
_C.TEST.GT_SCALE = False
_C.EVALUATORS = ("",)
_C.INPUT = CN()
_C.DATASETS = CN()
for _split in ("TRAIN", "TEST"):
    _C.DATASETS[_split] = CN()
    _C.DATASETS[_split].NAME = ""
    _C.DATASETS[_split].SPLIT = ""
    _C.DATASETS[_split].DATA_ROOT = ""
    _C.DATASETS[_split].IMG_WIDTH = 768
    _C.DATASETS[_split].IMG_HEIGHT = 384
    _C.DATASETS[_split].PREPROCESS = []
_C.DATALOADER = CN()
_C.DATALOADER.NUM_WORKERS = 6
_C.DATALOADER.SAMPLER_TRAIN = "DDPSampler"
_C.OUTPUT_DIR = "./output"
_C.SEED = -1
_C.CUDNN_BENCHMARK = False
_C.VIS_PERIOD = 0
_C.RUN_NAME = ""
_C.LOG_PERIOD = 20

# The hot-path keys of the two projects' Base.yaml (projects/MonoDepth2/configs/Base.yaml, projects/Supervised/configs/Base.yaml), as dict
# literals: /root/reference does not exist on the GPU box, so tests and bench.py build their configs from these instead of the YAML files
# (tests/test_config.py checks them against the files where the reference is present).
PROJECT_BASE = {
    "MonoDepth2": {
        "MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "MAX_DEPTH": 80},
        "LOSS": {"SSIM_WEIGHT": 0.85, "C1": 1e-4, "C2": 9e-4, "CLIP": 0.0, "AUTOMASK": True, "SMOOTHNESS_WEIGHT": 1e-3, "PHOTOMETRIC_REDUCE": "min",
                 "SUPERVISED_WEIGHT": 0.0, "VARIANCE_FOCUS": 0.85, "VAR_LOSS_WEIGHT": 0.0},
        "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}, {"NAME": "LoadDepth", "KEEP_ORIG": True}, {"NAME": "ClipDepth", "MAX_DEPTH": 80},
                                             {"NAME": "Resize", "IMG_W": 640, "IMG_H": 192}, {"NAME": "ToTensor"}]}},
        "SOLVER": {"IMS_PER_BATCH": 16, "DEPTH_LR": 2e-4, "POSE_LR": 2e-4, "LR_STEPS": (15,), "GAMMA": 0.1, "MAX_EPOCHS": 20, "CHECKPOINT_PERIOD": 1},
        "EVALUATORS": ("kitti_evaluator", "kitti_evaluator_0_30", "kitti_evaluator_30_50", "kitti_evaluator_50_80"),
        "TEST": {"GT_SCALE": True},
        "LOG_PERIOD": 20,
    },
    "Supervised": {
        "MODEL": {"META_ARCHITECTURE": "SupDepthModel", "MAX_DEPTH": 80},
        "LOSS": {"VARIANCE_FOCUS": 0.85},
        "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}, {"NAME": "LoadDepth", "KEEP_ORIG": True}, {"NAME": "ClipDepth", "MAX_DEPTH": 80},
                                             {"NAME": "KBCrop"}, {"NAME": "ToTensor"}]}},
        "SOLVER": {"IMS_PER_BATCH": 16, "DEPTH_LR": 1e-4, "DEPTH_END_LR": 1e-5, "MAX_EPOCHS": 50, "CHECKPOINT_PERIOD": 1},
        "EVALUATORS": ("kitti_evaluator", "kitti_evaluator_0_30", "kitti_evaluator_30_50", "kitti_evaluator_50_80"),
        "TEST": {"GT_SCALE": False},
        "LOG_PERIOD": 20,
    },
    # projects/MotionLearning/configs/resnet18_waymo.yaml over its Base_waymo.yaml: the model, loss and solver keys (the WaymoDepth dataset blocks are in
    # PROJECT_DATASETS below)
    "MotionLearningWaymo": {
        "MODEL": {"META_ARCHITECTURE": "MotionLearningModel", "MAX_DEPTH": 80, "WITH_MASK": True,
                  "DEPTH_NET": {"NAME": "GoogleResNetv2", "ENCODER_NAME": "18??", "UPSAMPLE_DEPTH": False, "LEARN_SCALE": False, "NORM": "randLN",
                                "NOISE_STDDEV": 0.5, "RAMPUP_ITERS": 10000},
                  "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "GROUP_NORM": False, "MASK_MOTION": True, "LEARN_SCALE": True,
                               "BURN_IN_ITERS": 20000, "SCALE_CONSTRAIN": "clip_ste"}},
        "LOSS": {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "CLIP": 0.0, "DEPTH_L1_WEIGHT": 0.0, "SMOOTHNESS_WEIGHT": 1e-3,
                 "SUPERVISED_WEIGHT": 0.0, "VARIANCE_FOCUS": 0.85, "VAR_LOSS_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0, "MOTION_SPARSITY_WEIGHT": 0.2,
                 "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False},
        "SOLVER": {"IMS_PER_BATCH": 16, "DEPTH_LR": 2e-4, "POSE_LR": 2e-4, "LR_STEPS": (200,), "GAMMA": 0.5, "MAX_EPOCHS": 200, "CHECKPOINT_PERIOD": 10,
                   "CLIP_GRAD": 10},
        "EVALUATORS": ("kitti_evaluator", "kitti_evaluator_0_30", "kitti_evaluator_30_50", "kitti_evaluator_50_80"),
        "TEST": {"GT_SCALE": True},
        "LOG_PERIOD": 20,
    },
    # projects/MonoDepth2/configs/resnet18_waymo.yaml and projects/Supervised/configs/resnet18_waymo.yaml over their Base_waymo.yaml: model, loss,
    # solver and TEST keys ("18pt" asks for ImageNet weights, as in the YAML: set ENCODER_NAME "18" to train from scratch)
    "MonoDepth2Waymo": {
        "MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "MAX_DEPTH": 80,
                  "DEPTH_NET": {"NAME": "DepthResNet", "ENCODER_NAME": "18pt", "UPSAMPLE_DEPTH": False}, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}},
        "LOSS": {"SSIM_WEIGHT": 0.85, "C1": 1e-4, "C2": 9e-4, "CLIP": 0.0, "AUTOMASK": True, "SMOOTHNESS_WEIGHT": 1e-3, "PHOTOMETRIC_REDUCE": "min",
                 "SUPERVISED_WEIGHT": 0.0, "VARIANCE_FOCUS": 0.85, "VAR_LOSS_WEIGHT": 0.0},
        "SOLVER": {"IMS_PER_BATCH": 16, "DEPTH_LR": 2e-4, "POSE_LR": 2e-4, "LR_STEPS": (40,), "GAMMA": 0.1, "MAX_EPOCHS": 50, "CHECKPOINT_PERIOD": 1},
        "EVALUATORS": ("kitti_evaluator", "kitti_evaluator_0_30", "kitti_evaluator_30_50", "kitti_evaluator_50_80"),
        "TEST": {"GT_SCALE": True},
        "LOG_PERIOD": 20,
    },
    "SupervisedWaymo": {
        "MODEL": {"META_ARCHITECTURE": "SupDepthModel", "MAX_DEPTH": 80, "DEPTH_NET": {"NAME": "DepthResNet", "ENCODER_NAME": "18pt", "UPSAMPLE_DEPTH": False}},
        "LOSS": {"VARIANCE_FOCUS": 0.85},
        "SOLVER": {"IMS_PER_BATCH": 16, "DEPTH_LR": 1e-4, "DEPTH_END_LR": 1e-5, "MAX_EPOCHS": 50, "CHECKPOINT_PERIOD": 1},
        "EVALUATORS": ("kitti_evaluator", "kitti_evaluator_0_30", "kitti_evaluator_30_50", "kitti_evaluator_50_80"),
        "TEST": {"GT_SCALE": False},
        "LOG_PERIOD": 20,
    },
}


def _waymo(split, preprocess, **kw):
    d = {"NAME": "WaymoDepth", "DATA_ROOT": f"/data2/data/waymo/{split}/image", "DEPTH_ROOT": f"/data2/data/waymo/{split}/depth",
         "SPLIT": f"/data2/data/waymo/infos/{split}_infos.pkl", "USE_CAMS": ["FRONT"]}
    d.update(kw)
    d["PREPROCESS"] = preprocess
    return d


# The DATASETS.TRAIN / DATASETS.TEST blocks of the three Waymo projects' Base_waymo.yaml (roots as the YAMLs have them: point DATA_ROOT, DEPTH_ROOT,
# MASK_ROOT and SPLIT at the local copy).  Kept apart from PROJECT_BASE and merged by get_project_cfg(project, datasets=True) only: models, losses
# and benchmarks that feed synthetic batches take the project without a dataset.
PROJECT_DATASETS = {
    "MotionLearningWaymo": {
        "TRAIN": _waymo("training", [{"NAME": "LoadImg", "WITH_CTX": True}, {"NAME": "LoadMask"}, {"NAME": "CropTopTo", "IMG_H": 1152},
                                              {"NAME": "Resize", "IMG_W": 320, "IMG_H": 192}, {"NAME": "RandomFlip"}, {"NAME": "RandomImageAug"}, {"NAME": "ToTensor"}],
                        MASK_ROOT="/data2/data/waymo/training/segmentation", DOWNSAMPLE=2, WITH_DEPTH=False, WITH_POSE=False, FORWARD_CONTEXT=1, STRIDE=1),
        "TEST": _waymo("validation", [{"NAME": "LoadImg"}, {"NAME": "LoadDepth", "KEEP_ORIG": True}, {"NAME": "ClipDepth", "MAX_DEPTH": 80},
                                              {"NAME": "CropTopTo", "IMG_H": 1152}, {"NAME": "Resize", "IMG_W": 320, "IMG_H": 192}, {"NAME": "ToTensor"}],
                       DOWNSAMPLE=20, WITH_DEPTH=False, WITH_POSE=False),
    },
    "MonoDepth2Waymo": {
        "TRAIN": _waymo("training", [{"NAME": "LoadImg", "WITH_CTX": True}, {"NAME": "CropTopTo", "IMG_H": 768}, {"NAME": "Resize", "IMG_W": 480, "IMG_H": 192},
                                              {"NAME": "RandomFlip"}, {"NAME": "RandomImageAug"}, {"NAME": "ToTensor"}],
                        DOWNSAMPLE=2, WITH_DEPTH=False, WITH_POSE=False, FORWARD_CONTEXT=1, BACKWARD_CONTEXT=1, STRIDE=1),
        "TEST": _waymo("validation", [{"NAME": "LoadImg"}, {"NAME": "LoadDepth", "KEEP_ORIG": True}, {"NAME": "ClipDepth", "MAX_DEPTH": 80},
                                              {"NAME": "CropTopTo", "IMG_H": 768}, {"NAME": "Resize", "IMG_W": 480, "IMG_H": 192}, {"NAME": "ToTensor"}],
                       DOWNSAMPLE=20, WITH_DEPTH=False, WITH_POSE=False),
    },
    # as in the YAML: this project trains on the validation split and tests on the training split
    "SupervisedWaymo": {
        "TRAIN": _waymo("validation", [{"NAME": "LoadImg"}, {"NAME": "LoadDepth"}, {"NAME": "ClipDepth", "MAX_DEPTH": 80}, {"NAME": "CropTopTo", "IMG_H": 768},
                                                {"NAME": "RandomCrop", "IMG_W": 704, "IMG_H": 352}, {"NAME": "RandomFlip"}, {"NAME": "RandomImageAug"}, {"NAME": "ToTensor"}],
                        WITH_DEPTH=True),
        "TEST": _waymo("training", [{"NAME": "LoadImg"}, {"NAME": "LoadDepth", "KEEP_ORIG": True}, {"NAME": "ClipDepth", "MAX_DEPTH": 80},
                                            {"NAME": "CropTopTo", "IMG_H": 768}, {"NAME": "ToTensor"}],
                       DOWNSAMPLE=20, WITH_DEPTH=True),
    },
}

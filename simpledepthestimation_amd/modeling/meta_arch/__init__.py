"""Meta architectures of the hot path.  Importing the three model modules registers their classes in META_ARCH_REGISTRY."""
from . import MonoDepth2 as _mono, MotionLearning as _motion, Supervised as _sup, build as _build

META_ARCH_REGISTRY, build_model = _build.META_ARCH_REGISTRY, _build.build_model
SupDepthModel, MonoDepth2Model, MotionLearningModel = _sup.SupDepthModel, _mono.MonoDepth2Model, _motion.MotionLearningModel

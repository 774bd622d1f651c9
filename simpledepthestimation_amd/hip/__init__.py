"""ctypes binding of libsde_hip.so + torch.autograd wrappers (tensor memory / streams are torch plumbing)."""
from . import present  # noqa: F401  (registers sde_depth_present: whoever binds the library binds every symbol the header declares)

from .camera import resize_img, resize_img_avgpool, scale_intrinsics, view_synthesis  # noqa: F401

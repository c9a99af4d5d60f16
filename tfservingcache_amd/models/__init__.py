from .builders import (build_half_plus_two, build_mlp, build_resnet50,
                       build_resnext, build_separable_cnn, build_bert,
                       build_unet, write_model_repo)  # noqa: F401

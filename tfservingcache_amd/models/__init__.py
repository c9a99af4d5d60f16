from .builders import (build_half_plus_two, build_mlp, build_resnet50,
                       build_resnext, build_separable_cnn, build_bert,
                       build_unet, build_deeplab, build_retrieval,
                       build_pooling_encoder, build_video_resnet,
                       build_unet3d, build_lstm_tagger, build_ssd_detector,
                       write_model_repo)  # noqa: F401

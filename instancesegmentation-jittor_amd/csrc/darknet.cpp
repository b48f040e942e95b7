// darknet.cpp -- the Darknet-53 trunk, DarkNetBackbone([1, 2, 8, 8, 4]): the backbone of yolact_darknet53_config (yolact.cpp) and of YOLOv3 (yolov3.cpp).
#include "engine.h"

namespace isegmi {

// Layers <prefix>_preconv.0, <prefix>layers.<L>.0.0 (the stride-2 3x3 that opens layer L) and <prefix>layers.<L>.<B>.{conv1, conv2} (block B >= 1); the
// outputs of layers 2-4 (strides 8, 16, 32: 256, 512, 1024 channels) -> C[0..2].  before_c3 (optional): the main stream waits on it before the first launch
// that overwrites C[0] -- the caller's fence against a reader of the previous forward's C maps.
int darknet_backbone(Engine& e, const std::string& prefix, const float* d_images, int N, Tensor* C, hipEvent_t before_c3) {
    if (e.fp16) { set_error("the Darknet53 backbone runs in fp32 only"); return ISEGMI_ERR_STATE; }
    // _preconv: 3x3 on the 3-channel image, via a zero-padded 32-channel copy; every conv is Conv + BN + LeakyReLU(0.1), a
    // block is 1x1 (C -> C/2) then 3x3 (C/2 -> C) with the shortcut added AFTER the activation (act 4)
    Tensor x4, x;
    TRY(eng_act(e, "input32", N, e.H, e.W, 32, &x4));
    TRY(pad_c3_c32_launch(d_images, (int64_t)N * e.H * e.W, x4.d, e.cur));
    TRY(eng_input_consumed(e));
    TRY(eng_conv(e, prefix + "_preconv.0", x4, 1, 1, 3, nullptr, "stem", &x));
    eng_mark(e, "stem");
    const int nblk[5] = {1, 2, 8, 8, 4};
    for (int li = 0; li < 5; ++li) {
        const std::string ln = prefix + "layers." + std::to_string(li);
        if (li == 2 && before_c3) HIP_TRY(hipStreamWaitEvent(e.stream, before_c3, 0));
        Tensor y;
        TRY(eng_conv(e, ln + ".0.0", x, 2, 1, 3, nullptr, ln + ".down", &y));
        x = y;
        for (int b = 1; b <= nblk[li]; ++b) {
            const std::string nm = ln + "." + std::to_string(b);
            Tensor t1;
            TRY(eng_conv(e, nm + ".conv1", x, 1, 0, 3, nullptr, nm + ".t1", &t1));
            TRY(eng_conv(e, nm + ".conv2", t1, 1, 1, 4, &x, nm + ".out", &y));
            x = y;
        }
        if (li >= 2) C[li - 2] = x;
        if (li >= 1) eng_mark(e, li == 1 ? "layer1" : li == 2 ? "layer2" : li == 3 ? "layer3" : "layer4");
    }
    return ISEGMI_OK;
}

// The trunk of yolov3-tiny: <prefix>conv0..6, 3x3 + BN + LeakyReLU(0.1) to 16 (stored as 32: the host pads conv0's rows and conv1's input
// channels with zeros, as the image is padded), 32, 64, 128, 256, 512, 1024 channels; a darknet 2 / 2 max-pool after conv0..4, a 2 / 1 pool after conv5.
// *skip = conv4's output (256 channels, stride 16), *top = conv6's (1024, stride 32).
int darknet_tiny_backbone(Engine& e, const std::string& prefix, const float* d_images, int N, int zero_pad, Tensor* skip, Tensor* top) {
    if (e.fp16) { set_error("the yolov3-tiny trunk runs in fp32 only"); return ISEGMI_ERR_STATE; }
    Tensor x;
    TRY(eng_act(e, "input32", N, e.H, e.W, 32, &x));
    TRY(pad_c3_c32_launch(d_images, (int64_t)N * e.H * e.W, x.d, e.cur));
    TRY(eng_input_consumed(e));
    for (int i = 0; i < 7; ++i) {
        const std::string nm = "conv" + std::to_string(i);
        Tensor y;
        TRY(eng_conv(e, prefix + nm, x, 1, 1, 3, nullptr, "trunk." + nm, &y));
        if (i == 4) *skip = y;
        x = y;
        if (i < 6) {
            const int stride = i < 5 ? 2 : 1;
            TRY(eng_act(e, "trunk.pool" + std::to_string(i), N, (y.H - 1) / stride + 1, (y.W - 1) / stride + 1, y.C, &x));
            OpScope op(e, e.cur, "maxpool_darknet", (double)(y.numel() + x.numel()) * 4);
            TRY(maxpool_darknet_launch(y.d, N, y.H, y.W, y.C, 2, stride, zero_pad, x.d, e.cur));
        }
    }
    *top = x;
    eng_mark(e, "trunk");
    return ISEGMI_OK;
}

}  // namespace isegmi

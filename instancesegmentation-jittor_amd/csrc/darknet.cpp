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

}  // namespace isegmi

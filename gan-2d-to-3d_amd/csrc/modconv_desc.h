// modconv_desc.h — what the two implicit-GEMM convolution kernels (modconv.hip: fp32 operands,
// modconv_f16.hip: fp16 operands) and their launcher (conv_launch in modconv.hip) share: the launch
// descriptor.
#pragma once
#include "g2s_common.h"

namespace g2s {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));

constexpr int NTHREADS = 256;

struct ConvClass {  // one output-parity class (a single class for gather geometries)
    int OH, OW;     // class output extent
    int T;          // taps in this class
    int oy0, ox0;   // offset of the class in the full output
    int tab[25];    // per tap: (dy + 8) | (dx + 8) << 8 | wtap << 16
};

static inline int pack(int dy, int dx, int wt) { return (dy + 8) | ((dx + 8) << 8) | (wt << 16); }  // a ConvClass::tab entry

struct ConvDesc {
    const float *x, *w, *in_scale, *out_scale;
    float *y;
    int B, Cr, M;        // batch, reduction channels, output channels
    int H, W;            // input spatial size
    int OHf, OWf;        // full output spatial size
    int w_ms, w_ks;      // strides (in floats) of the m index and the reduction-channel index in w
    int is;              // input stride of the gather (1 or 2)
    int os;              // output stride of a class (1, or 2 for the polyphase classes)
    int ncls;
    int splitk;
    int w_bytes;         // size of ONE group's w in bytes (buffer-resource range)
    // Grouped launch (two structurally identical trained nets run as one, their channels side by
    // side: op/conv.py PairConvFunction): `groups` independent convolutions of Cr -> M channels;
    // x has Cx = groups * Cr channels per sample, y has My = groups * M, w / bias hold the groups
    // back to back.  groups = 1: Cx = Cr, My = M.
    int groups, Cx, My;
    int cls_splitk[4];   // split-K slices of each class (<= splitk = grid.y): lighter classes get fewer
    const float *bias;   // [M] added after out_scale, or NULL
    // StyledConv's NoiseInjection (stylegan2-pytorch/model.py:294-305,349-355) in the epilogue: + noise_w[0] *
    // noise[oy * OWf + ox], one [OHf, OWf] map for all samples and channels; NULL: none
    const float *noise, *noise_w;
    int act;             // 0: none, 1: leaky-ReLU(alpha) * gain applied after the bias
    float act_alpha, act_gain;
    ConvClass cls[4];
};

// The fp16-operand kernel (modconv_f16.hip) on a descriptor conv_launch has filled: tile `pick` 2 = 64x64, else
// 128x128.  Launches only (the caller checks the launch); G2S_ERR_INVALID for a geometry it does not serve.
int modconv_f16_launch(const ConvDesc &d, dim3 grid, int pick, hipStream_t st);

}  // namespace g2s

// The block activation (--act) in one place: OrnAct<ACT>::f / df are what the 16-bit kernels call (fast pair), f_exact / df_exact what
// the fp32 path calls.  ACT is a compile-time parameter of every kernel that evaluates the activation (ORN_ACT_* of include/orn.h);
// launchers switch on the run-time `act` with ORN_ACT_SWITCH.
#pragma once
// (included by orn_common.h behind the SiLU helpers it forwards to)

template <int ACT> struct OrnAct;

// swish: the helpers of orn_common.h, unchanged -- the swish instantiation of a kernel is the kernel of before
template <> struct OrnAct<ORN_ACT_SWISH> {
    static __device__ __forceinline__ float f(float z) { return orn_silu(z); }
    static __device__ __forceinline__ float df(float z) { return orn_silu_grad(z); }
    static __device__ __forceinline__ float f_exact(float z) { return orn_silu_exact(z); }
    static __device__ __forceinline__ float df_exact(float z) { return orn_silu_grad_exact(z); }
};

// GELU, nn.GELU() without the tanh approximation:
//   gelu(z)  = 0.5 z erfc(-z / sqrt 2)
//   gelu'(z) = 0.5 erfc(-z / sqrt 2) + z exp(-z^2 / 2) / sqrt(2 pi),   |gelu'| <= 1.129
// erfc, not 1 + erf: the latter loses the negative tail to cancellation (5.8 ulp16 of gelu(z) over the finite fp16 z against 0.002).
// z -> -inf: erfc -> 0 and the product is -0; z^2 may overflow to +inf, exp(-inf) = 0 and z * 0 = 0 for every finite z.
// The fast pair is the exact pair: no cheaper erfc has been put through the sweep of tests/test_gpu_act_eval.py.
template <> struct OrnAct<ORN_ACT_GELU> {
    static __device__ __forceinline__ float f_exact(float z) { return 0.5f * z * erfcf(-0.70710678118654752440f * z); }
    static __device__ __forceinline__ float df_exact(float z)
    {
        return fmaf(0.5f, erfcf(-0.70710678118654752440f * z), z * expf(-0.5f * z * z) * 0.39894228040143267794f);
    }
    static __device__ __forceinline__ float f(float z) { return f_exact(z); }
    static __device__ __forceinline__ float df(float z) { return df_exact(z); }
};

static inline bool orn_act_known(int act) { return act == ORN_ACT_SWISH || act == ORN_ACT_GELU; }

// ORN_ACT_SWITCH(act, ACT_, stmt): stmt with the constant ACT_ bound to the run-time act (checked by the caller: orn_act_known)
#define ORN_ACT_SWITCH(act_, ACT_, ...)                                  \
    do {                                                                 \
        if ((act_) == ORN_ACT_GELU) { constexpr int ACT_ = ORN_ACT_GELU; __VA_ARGS__; } \
        else { constexpr int ACT_ = ORN_ACT_SWISH; __VA_ARGS__; }         \
    } while (0)

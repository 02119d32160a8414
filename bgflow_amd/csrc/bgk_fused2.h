/* bgk_fused2.h -- internal: launcher of the second-generation split-f16 coupling kernel (bgk_fused2.hip) */
#ifndef BGK_FUSED2_H
#define BGK_FUSED2_H
#include <stdint.h>

#define BGK_MAX_COND 3
/* several conditioning tensors [B, w_i] standing for their concatenation (host-side table of device pointers; NULL / n <= 1: the
 * single (cond, ldc, d_c) tensor of the launcher's own arguments) */
struct BgkCondSegs { const float* ptr[BGK_MAX_COND]; int64_t ld[BGK_MAX_COND]; int32_t w[BGK_MAX_COND]; int32_t n; };

/* the spline's domain [left, right] x [bottom, top], its minimal bin sizes / slope and the identity-init flag: built ONCE, by field name,
 * in every extern "C" entry that receives the eight scalars, and passed on as a whole */
struct BgkSplineBox { double left, right, bottom, top, min_bin_width, min_bin_height, min_derivative; int32_t identity_init; };

/* one call of a fused spline coupling launcher (bgk_fused.hip::launch_h2 and the second-generation launchers below); filled by field name */
struct BgkRqsDenseCall {
    const char* what;                                  /* the entry point, for error texts */
    const float* cond; int64_t ldc; int32_t d_c, periodic;
    const BgkCondSegs* segs;                           /* several conditioning tensors (NULL / n <= 1: the tensor (cond, ldc, d_c)) */
    const void *A0p, *A1p, *A2p; float c0, c1, c2; const float* cs_dev;
    int32_t act; const float* y; int64_t ldy; int64_t B; int32_t d; uint64_t circ_mask; int32_t inverse;
    BgkSplineBox box;
    float* out; int64_t ldo; float* dlogp; int32_t accumulate; int32_t* bin_idx; int32_t* oob_count; void* stream;
    /* row order of the output-layer operand A2p -- 1 = bgk_pack_rqs_columns, 2 = bgk_pack_rqs_columns_v(row_order = 2): the split-f16
     * inference instance then keeps the spline's widths / heights in the accumulator registers (the other instances take 1 only) */
    int32_t row_order;
    /* training forward only: z0, z1 [B, 128] and params [B, ldp] written for the backward (params NULL: not written; src_col NULL: element-major) */
    float *z0, *z1, *params; int64_t ldp; const int32_t* src_col;
};
int bgk_launch_rqs_dense_h2v2(const BgkRqsDenseCall& c);          /* split-f16 inference (bgk_fused2.hip) */
int bgk_launch_rqs_dense_h2v2_train(const BgkRqsDenseCall& c);    /* the training forward (bgk_fused2_train.hip): same kernel + the save part */
int bgk_launch_rqs_dense_h2v2_bf16(const BgkRqsDenseCall& c);     /* reduced-precision mode "bf16" (bgk_fused2_bf16.hip): one bf16 MFMA per product */

/* spline backward of a layer the training forward ran WITHOUT writing its parameters (params == NULL there): the output layer of
 * the conditioner redone from z1 on the matrix cores, bgk_rqs_vjp_element on every element (bgk_fused2_train.hip) */
struct BgkRqsBwdCall {
    const char* what; const float* z1; const void* A2p; float c2; const float* cs_dev; int32_t act;
    const float* y; int64_t ldy; int64_t B; int32_t d; uint64_t circ_mask; int32_t inverse;
    BgkSplineBox box;
    const float* g_out; int64_t ldgo; const float* g_dlogp; float* g_y; int64_t ldgy; float* g_params; int64_t ldgp; float* g_absmax; void* stream;
};
int bgk_launch_rqs_bwd_recompute(const BgkRqsBwdCall& c);

/* one conditioner network of an affine coupling: packed operands of layer 0, the hidden layer(s) and the output layer with their scales
 * (A0 == NULL: no such network; A1b == NULL: two hidden layers, else three) and its activation code */
struct BgkAffNetOps { const void *A0, *A1, *A1b, *A2; float c0, c1, c1b, c2; int32_t act; };

/* one call of a fused affine coupling launcher (bgk_fused_affine.hip::affine_dense_launch and the launchers below); filled by field name */
struct BgkAffDenseCall {
    const float* cond; int64_t ldc; int32_t d_c, periodic;
    const BgkCondSegs* segs;                           /* several conditioning tensors (NULL / n <= 1: the tensor (cond, ldc, d_c)) */
    BgkAffNetOps shift, scale;
    const float* log_alpha; int32_t preserve_volume, is_circular, inverse;
    const float* y; int64_t ldy; int64_t B; int32_t d;
    float* out; int64_t ldo; float* dlogp; int32_t accumulate; void* stream;
};

/* affine coupling layer with conditioners of width 128 (two or three hidden layers) on the same event-threaded GEMM stream
 * (bgk_fused2.hip); BGK_EUNSUPPORTED for activation pairs it has no instance for */
int bgk_launch_affine_dense_v2(const BgkAffDenseCall& c);

/* the training forward of the affine layer (bgk_fused2_afftrain.hip): the same kernel (two hidden layers) + what the backward reads --
 * per network the scaled pre-activations z0, z1 [B, ldz] and its output rows (mu; the scale values before tanh) [B, ldms];
 * s_cs / t_cs: device scale tables of the packed operands (NULL: the c values of the call) */
struct BgkAffTrainSave { const float* s_cs; float* s_z0; float* s_z1; const float* t_cs; float* t_z0; float* t_z1; float* mu; float* s_raw; int64_t ldms;
                         int64_t ldz; };      /* row pitch of the z arrays: 128, or 64 when every hidden layer has <= 64 units */
int bgk_launch_affine_dense_v2_train(const BgkAffTrainSave* save, const BgkAffDenseCall& c);

/* 2 (default): coupling_rqs_dense_h2v2_kernel for the split-f16 path (inference and training forward); 1: the first-generation kernel */
extern int bgk_h2_variant;
/* 2 (default): bgk_coupling_rqs_dense_h2_backward evaluates the element VJP's softmax / knots on the hardware exp2 / rcp forms (like the
 * fused forward it belongs to); 1: on the deterministic forms of bgk_rqs_backward (bit-identical gradients with the saved-parameter path) */
extern int bgk_rc_vjp_variant;

#endif

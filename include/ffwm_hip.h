/*
 * ffwm_hip.h -- C ABI of libffwm_hip.so, the MI355X (gfx950) implementation of the
 * flow-guided feature-warping hot path of csyxwei/FFWM.
 *
 * This is the drop-in boundary: each entry point below replaces one native function the
 * reference binds through pybind11 (citations are into the reference repository).  The
 * reference passes `at::Tensor&`; here every tensor is a raw device pointer to a
 * CONTIGUOUS NCHW buffer plus its sizes, so the library has no PyTorch dependency:
 *
 *   ffwm_block_extractor_forward    <- block_extractor_cuda.forward     cuda/block_extractor/block_extractor_cuda.cc:5-12
 *   ffwm_block_extractor_backward   <- block_extractor_cuda.backward    cuda/block_extractor/block_extractor_cuda.cc:14-25
 *   ffwm_local_attn_reshape_forward <- local_attn_reshape_cuda.forward  cuda/local_attn_reshape/local_attn_reshape_cuda.cc:5-11
 *   ffwm_local_attn_reshape_backward<- local_attn_reshape_cuda.backward cuda/local_attn_reshape/local_attn_reshape_cuda.cc:13-21
 *   ffwm_resample2d_forward         <- resample2d_cuda.forward          cuda/resample2d_package/resample2d_cuda.cc:6-14
 *   ffwm_resample2d_backward        <- resample2d_cuda.backward         cuda/resample2d_package/resample2d_cuda.cc:16-26
 *   ffwm_warp_forward / _backward   <- WarpNet.forward (F.grid_sample)  models/base_networks.py:168-173, fused with the
 *                                      flip + concat of FFWM.forward    models/base_networks.py:326-329
 *   ffwm_guided_filter_*            <- GuidedFilter.forward             models/external_function.py:239-277
 *   ffwm_affine_regularization      <- AffineRegularizationLoss.__call__ models/losses.py:200-219
 *   ffwm_correlation_colmax         <- max(bmm(source, target), dim=1)  models/losses.py:347-353
 *   ffwm_correlation_colmax_split   <- the same on bf16 MFMA with a hi/lo operand split (opt-in)
 *   ffwm_sampling_correctness       <- PerceptualCorrectness.calculate_loss (warp, cosine, exp, mask, sums)  models/losses.py:341-371
 *   ffwm_landmark_loss              <- MultiScaleLDLoss / LandmarkLoss, every scale and its gradient in one call  models/losses.py:61-74,114-126
 *   ffwm_block_attention_*          <- avg_pool2d(BlockExtractor * LocalAttnReshape)  (composition of the ops above)
 *   ffwm_spectral_norm_*            <- torch.nn.utils.spectral_norm hooks models/base_networks.py:5,218-264,381-413
 *   ffwm_conv3x3_wgrad[_block]      <- convolution_backward grad_weight / grad_bias of the nn.Conv2d(., ., 3, 1, 1) layers
 *   ffwm_bn_lrelu_*                 <- nn.BatchNorm2d (training) + nn.LeakyReLU of the conv blocks  models/base_networks.py:12-31
 *   ffwm_mfm_*                      <- mfm.forward (split + max)        lightcnn/light_cnn.py
 *   ffwm_bias_relu_forward          <- conv bias add + nn.ReLU of VGG19  models/losses.py:398-519
 *   ffwm_adam_step                  <- torch.optim.Adam.step            models/ffwm_model.py:46-49,151-160
 *   ffwm_sgd_step                   <- torch.optim.SGD.step, one group per tensor  lightcnn/finetune.py:74-90
 *   ffwm_grad_health                <- the total norm of torch.nn.utils.clip_grad_norm_ and an isfinite check, per network (no
 *                                      counterpart in the reference, whose loop looks at no gradient)
 *   ffwm_adam_step_guarded          <- clip_grad_norm_ + `if isfinite: optimizer.step()` with the decision on the device
 *   ffwm_softmax_xent               <- nn.CrossEntropyLoss + accuracy(output, target, (1, 5))  lightcnn/finetune.py:109,152-159
 *   ffwm_l1_multi                   <- the w * F.l1_loss(x * m, y * m) terms of backward_G   models/ffwm_model.py:107-139
 *   ffwm_conv2d_wgrad[_tiled]       <- convolution_backward grad_weight of the stride-2 / transposed / small-plane convs
 *   ffwm_visuals                    <- tensor2im / tensor2mask / tensor2flow / tensor2att + flow2img   util/util.py:10-70, util/flow_util.py:23-153
 *
 * Conventions
 *   - dtype: FFWM_F32 or FFWM_F64 (the reference dispatches AT_DISPATCH_FLOATING_TYPES).
 *   - stream: a hipStream_t passed as void* (NULL = the null stream).  Launches are
 *     asynchronous, never synchronise, never allocate; the library keeps no tensor state.
 *     (One stated exception: ffwm_grad_health reads its segment table back, and waits for the stream, when that stream is
 *     not being captured.)
 *   - The kernels run on the CURRENT HIP device of the calling thread; the caller selects the
 *     device that owns the pointers (one process per GPU in this project).
 *   - Ownership: the caller allocates every output.  Forward outputs are fully overwritten
 *     (no zero-fill needed).  Gradient outputs marked "+=" are accumulated into, exactly as
 *     the reference's atomicAdd kernels do, so the caller zero-fills them first
 *     (models/external_function.py:49-50,96,137-138).  A NULL gradient pointer skips that
 *     gradient.
 *   - Return: 0 on success, a negative ffwm_status otherwise; ffwm_last_error() returns a
 *     thread-local message.  (The reference returns 1 unconditionally and checks nothing.)
 *   - Index arithmetic is 64-bit for flat offsets (the reference overflows 32-bit `int`
 *     above 2^31 elements); a single H*W plane must stay below 2^31 elements.
 */
#ifndef FFWM_HIP_H_
#define FFWM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFWM_ABI_VERSION 5

typedef enum {
    FFWM_OK = 0,
    FFWM_ERR_ARG = -1,     /* NULL pointer, non-positive size, bad kernel_size/dilation */
    FFWM_ERR_DTYPE = -2,   /* dtype is not FFWM_F32 / FFWM_F64 */
    FFWM_ERR_SIZE = -3,    /* a plane exceeds 2^31 elements */
    FFWM_ERR_LAUNCH = -4   /* HIP reported a launch error */
} ffwm_status;

typedef enum { FFWM_F32 = 0, FFWM_F64 = 1 } ffwm_dtype;

int ffwm_abi_version(void);
const char* ffwm_last_error(void);

/* out[B,C,k*Hf,k*Wf][b,c,yf*k+i,xf*k+j] = bilinear(source[b,c], yf + flow[b,1,yf,xf] + i - k/2,
 *                                                  xf + flow[b,0,yf,xf] + j - k/2)
 * index-clamped border, weights from the unclamped fraction.
 * source[B,C,Hs,Ws], flow_field[>=B,2,Hf,Wf] (pixel units, ch0 = x, ch1 = y).
 * Reference: block_extractor_kernel.cu:21-85. */
int ffwm_block_extractor_forward(const void* source, const void* flow_field, void* output,
                                 int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf,
                                 int64_t Wf, int kernel_size, int dtype, void* stream);

/* grad_source[B,C,Hs,Ws] += 4-tap scatter of grad_output; grad_flow_field[B,2,Hf,Wf] += sum over
 * c and the k x k window of grad_output * d(bilinear)/d(x,y).  Either may be NULL.
 * Reference: block_extractor_kernel.cu:89-170. */
int ffwm_block_extractor_backward(const void* source, const void* flow_field,
                                  const void* grad_output, void* grad_source,
                                  void* grad_flow_field, int64_t B, int64_t C, int64_t Hs,
                                  int64_t Ws, int64_t Hf, int64_t Wf, int kernel_size,
                                  int dtype, void* stream);

/* out[B,1,k*H,k*W][b,0,y,x] = inputs[B,k*k,H,W][b,(y%k)*k + x%k, y/k, x/k].
 * Reference: local_attn_reshape_kernel.cu:21-61. */
int ffwm_local_attn_reshape_forward(const void* inputs, void* output, int64_t B, int64_t H,
                                    int64_t W, int kernel_size, int dtype, void* stream);

/* Inverse permutation.  accumulate != 0: grad_inputs += (reference semantics, atomicAdd into a
 * zero-filled buffer, local_attn_reshape_kernel.cu:66-108); accumulate == 0: grad_inputs is
 * overwritten (no zero-fill, half the traffic -- identical result on a zero-filled buffer). */
int ffwm_local_attn_reshape_backward(const void* grad_output, void* grad_inputs, int64_t B,
                                     int64_t H, int64_t W, int kernel_size, int accumulate,
                                     int dtype, void* stream);

/* grad_output through its ELEMENT STRIDES (ABI 5).  The reference's kernels index gradOutput with DIM3_INDEX and the tensor's own strides
 * (cuda/block_extractor/block_extractor_kernel.cu:8-15, local_attn_reshape_kernel.cu:8-15, resample2d_kernel.cu:8-15) and its Functions
 * throw the result of grad_output.contiguous() away (models/external_function.py:46-47,93-94,132-133), so a pybind module that replaces
 * the reference's must take an expanded / permuted / sliced gradient as it comes.  grad_output_strides[4] = (batch, channel, row, column)
 * strides in elements, all >= 0, column stride != 0; NULL or the contiguous NCHW strides = the entry points above (the tuned kernels).
 * Any other layout runs the per-element kernels: the reference's own decomposition -- correct for every view, not a tuned path.
 * Everything else as in the plain entry points (ffwm_block_extractor_backward, ffwm_local_attn_reshape_backward, ffwm_resample2d_backward). */
int ffwm_block_extractor_backward_strided(const void* source, const void* flow_field, const void* grad_output,
                                          const int64_t* grad_output_strides, void* grad_source, void* grad_flow_field, int64_t B,
                                          int64_t C, int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf, int kernel_size, int dtype,
                                          void* stream);
int ffwm_local_attn_reshape_backward_strided(const void* grad_output, const int64_t* grad_output_strides, void* grad_inputs, int64_t B,
                                             int64_t H, int64_t W, int kernel_size, int accumulate, int dtype, void* stream);
int ffwm_resample2d_backward_strided(const void* input1, const void* input2, const void* grad_output,
                                     const int64_t* grad_output_strides, void* grad_input1, void* grad_input2, int64_t B, int64_t C,
                                     int64_t Hi, int64_t Wi, int64_t H, int64_t W, int kernel_size, int dilation,
                                     int reference_quirk, int dtype, void* stream);

/* Gaussian-weighted kernel_size x kernel_size tap resampler.  input1[>=B,C,Hi,Wi],
 * input2[B,3,H,W] = (dx, dy, sigma) in pixels, out[B,C,H,W].
 * Reference: resample2d_kernel.cu:21-95.  kernel_size even >= 2, dilation >= 1. */
int ffwm_resample2d_forward(const void* input1, const void* input2, void* output, int64_t B,
                            int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                            int kernel_size, int dilation, int dtype, void* stream);

/* grad_input1[B,C,Hi,Wi] += scatter (resample2d_kernel.cu:98-202); grad_input2[B,3,H,W] is
 * OVERWRITTEN (resample2d_kernel.cu:204-330).  Either gradient may be NULL.
 * reference_quirk is a word of two FLAGS:
 *   bit 0 (value 1): the quirk -- keep the reference's `alpha = xf - int(xf)` truncation in the grad_input1 weights (:137-138);
 *                    clear: floor (the true gradient).
 *   bit 1 (value 2, ABI 5): overwrite -- grad_input1 arrives UNINITIALISED and is overwritten: the owned-tile kernels store every
 *                    cell exactly once (no zero-fill by the caller, no atomics on the regular path), every other path clears the
 *                    buffer itself first.  (With an empty grid nothing is launched: ffwm_amd.ops clears the buffer itself.)
 * A pixel whose NT x NT weight products all underflow (the reference's 16-product sum is 0) adds nothing, on every path.
 *
 * Precision of the SCATTER outputs (grad_input1 here; grad_source of the block extractor and block attention, grad_feat of the warp):
 * fp32 paths that accumulate in 32-bit fixed-point LDS cells scale a cell by a power of two taken from the largest gradient of its
 * CHANNEL among the pixels of the block that owns it.  For a cell with contributions w_i g_i (w_i >= 0), at every finite cell
 *     |got - ref| <= rho * sum_i |w_i g_i|  +  eta * L  (+ 1e-38),   rho = 2^-16, eta = 2^-12,
 * with ref the exact sum and L the largest |g| of the same channel within reach of the cell (the block's pixel region: 64 x 48
 * pixels for the resample2d owned tiles, 64 x 32 windows plus halo for the block extractor).  Non-finite cells sit exactly where
 * the reference's float atomics put them.  A flow that CONTRACTS many pixels onto one cell scales eta with the counted population.
 * (tests/scatter_bounds.py derives the two constants; the fp32 reference itself meets the bound with rho / 4 and eta = 0.) */
int ffwm_resample2d_backward(const void* input1, const void* input2, const void* grad_output,
                             void* grad_input1, void* grad_input2, int64_t B, int64_t C,
                             int64_t Hi, int64_t Wi, int64_t H, int64_t W, int kernel_size,
                             int dilation, int reference_quirk, int dtype, void* stream);

/* WarpNet: out[b,c,y,x] = grid_sample(feat[B,C,Hi,Wi], flow[B,2,H,W]) bilinear, zeros padding,
 * align_corners=False; flow = normalised absolute coordinates, ch0 = x, ch1 = y.
 * flipcat != 0: out is [B,2C,H,W] = cat(w, flip(w, dim 3)) (one read, two writes instead of
 * grid_sample + flip + cat).  Reference: models/base_networks.py:168-173,326-329.
 * Non-finite values of feat: a NaN or +-Inf cell reaches exactly the outputs that have it as a VALID corner, a corner of weight 0
 * included (the reference multiplies); a zero-padded corner is no tap, and a pixel without a valid corner is 0 whatever feat
 * holds.  (The LDS-staged tiles broke the last clause until the forward got its per-element bounds: such a pixel read the first
 * four cells of its tile's staged box with weight 0, so a NaN there became a NaN band in the padding.)
 * Per element |out - exact| <= 2^-19 sum_corners |w s| + the fp32 rounding of the unnormalised coordinate
 * (tests/sample_forward_bounds.py; the fp32 reference itself: a quarter of that). */
int ffwm_warp_forward(const void* feat, const void* flow, void* output, int64_t B, int64_t C,
                      int64_t Hi, int64_t Wi, int64_t H, int64_t W, int flipcat, int dtype,
                      void* stream);

/* grad_feat[B,C,Hi,Wi] += ; grad_flow[B,2,H,W] += .  Either may be NULL.  grad_output is
 * [B,C,H,W] or, with flipcat bit 0, [B,2C,H,W].  flipcat bit 1 (value 2, ABI 4): grad_feat is UNINITIALISED memory and is produced
 * whole -- the caller's zero-fill is saved (and, on the owned-tile path of planes beyond LDS, the read of it); grad_flow still
 * accumulates.  A pixel without a valid corner adds nothing to grad_flow, whatever feat and grad_output hold (the LDS-staged
 * d(flow) tiles used to add 0 x the first cells of the tile's box: NaN beside a non-finite cell). */
int ffwm_warp_backward(const void* feat, const void* flow, const void* grad_output,
                       void* grad_feat, void* grad_flow, int64_t B, int64_t C, int64_t Hi,
                       int64_t Wi, int64_t H, int64_t W, int flipcat, int dtype, void* stream);

/* Several independent warps in one call (at most a few launches): FFWM issues its warps in groups -- the eight 32 x 32
 * part crops of models/ffwm_model.py:84-88, the three illumination warps of models/losses.py:149, the three
 * warp-attention levels of models/base_networks.py:323-333 -- whose members are individually launch-bound.  Same
 * semantics per problem as ffwm_warp_forward / ffwm_warp_backward (grad_feat / grad_flow accumulate, either may be NULL;
 * forward ignores the three gradient fields).  All problems share flipcat and dtype. */
typedef struct ffwm_warp_problem {
    const void* feat;        /* [B,C,Hi,Wi] */
    const void* flow;        /* [B,2,H,W] */
    void* output;            /* forward: [B,C,H,W] or [B,2C,H,W] */
    const void* grad_output; /* backward */
    void* grad_feat;         /* backward, may be NULL */
    void* grad_flow;         /* backward, may be NULL */
    int64_t B, C, Hi, Wi, H, W;
} ffwm_warp_problem;
int ffwm_warp_multi_forward(const ffwm_warp_problem* problems, int n, int flipcat, int dtype, void* stream);
int ffwm_warp_multi_backward(const ffwm_warp_problem* problems, int n, int flipcat, int dtype, void* stream);

/* ---- the L1 terms of the generator loss in one launch (csrc/l1_loss.hip) ------------------------
 * models/ffwm_model.py:107-139 (backward_G) sums ~25 terms  w * F.l1_loss(x * m, y * m)  -- pixel loss :112-115, PerceptualLoss
 * (models/losses.py:293-320), MSL1Loss (:130-157), IdentityLoss (:76-112).  A problem is one term:
 *     out[slot] += scale * sum_i | x[i] * m[mi] - y[i] * m[mi] |      (scale = w / numel; mask NULL: m = 1)
 * with the mask broadcast over the channels: x [B, C, H, W] (n = B*chw elements, chw = C*H*W), mask [B, 1, H, W] (hw = H*W).
 * Forward (grad_out NULL): out[n_slots] is accumulated into (zero-fill it).  Backward (grad_out[n_slots] given):
 * grad_x = grad_out[slot] * scale * sign(x m - y m) * m is written for every problem (y is data: no gradient). */
typedef struct ffwm_l1_problem {
    const void* x;
    const void* y;
    const void* mask;       /* may be NULL */
    void* grad_x;           /* backward only */
    int64_t n, chw, hw;
    double scale;
    int slot;
} ffwm_l1_problem;
int ffwm_l1_multi(const ffwm_l1_problem* problems, int n, void* out, const void* grad_out, int n_slots, int dtype, void* stream);

/* ---- batched spectral normalisation of conv weights (netG / netD) -----------------------------
 * Replaces the per-layer hook of torch.nn.utils.spectral_norm that the reference wraps around every
 * convolution of FFWM and MSDiscriminator (models/base_networks.py:5,218-264,381-413):
 *     power_iterations x { v = normalize(W^T u); u = normalize(W v) };  sigma = u . (W v);
 *     weight_sn = W / sigma                         with W = weight.view(rows = Cout, cols = -1)
 * Three launches handle FFWM_SN_MAX_LAYERS layers (grids over (layer, chunk) pairs).  power_iterations
 * is 0 or 1 (the hook's default).  u[rows] and v[cols] are
 * updated IN PLACE (as the hook does in training mode) and copied to u_saved / v_saved, because a
 * later forward call may overwrite them before this call's backward runs (the hook clones them for
 * the same reason); power_iterations = 0 is the eval-mode behaviour (stored u, v).  wv[rows] is caller-provided scratch, sigma[1] receives sigma (needed by
 * the backward).  The `layers` array lives in HOST memory; all pointers inside are device pointers. */
#define FFWM_SN_MAX_LAYERS 32
typedef struct {
    const void* weight;   /* [rows, cols] */
    void* u;              /* [rows]  in/out */
    void* v;              /* [cols]  in/out */
    void* wv;             /* [rows]  scratch */
    void* weight_sn;      /* [rows, cols] out */
    void* sigma;          /* [1] out */
    void* u_saved;        /* [rows] out: the u this call normalised with (for its backward); may be NULL */
    void* v_saved;        /* [cols] out: likewise */
    int rows, cols;
} ffwm_sn_layer;

int ffwm_spectral_norm_forward(const ffwm_sn_layer* layers, int n_layers, int power_iterations,
                               double eps, int dtype, void* stream);

/* grad_weight = grad_weight_sn / sigma - (<grad_weight_sn, weight> / sigma^2) u v^T   (OVERWRITTEN;
 * u, v are constants, exactly as in the hook, where the power iteration runs under no_grad). */
typedef struct {
    const void* weight;          /* [rows, cols] */
    const void* u;               /* [rows] */
    const void* v;               /* [cols] */
    const void* sigma;           /* [1] */
    const void* grad_weight_sn;  /* [rows, cols] */
    void* grad_weight;           /* [rows, cols] out */
    void* partials;              /* scratch, ceil(rows*cols / 8192) elements */
    int rows, cols;
} ffwm_sn_grad_layer;

int ffwm_spectral_norm_backward(const ffwm_sn_grad_layer* layers, int n_layers, int dtype,
                                void* stream);

/* ---- guided filter (illumination-adaption path) ------------------------------------------------
 * out = GuidedFilter(r, eps)(x, y) of models/external_function.py:239-277 (box filters as cumsum
 * differences, :164-193), per [H, W] plane; x, y, out are [planes = B*C, H, W] contiguous with
 * c_x == c_y (the only way FFWM calls it: models/ffwm_model.py:57-59,81,104-105).  H, W <= 128
 * (these argument lists carry no workspace for longer lines: ffwm_guided_filter_*_general below), H > 2r+1, W > 2r+1.  `saved` [5, planes, H, W] receives mean_x, mean_y, A, var_x+eps, mean_A for the
 * backward.  Four launches (column pass / row pass + pointwise stage, twice), each over planes x W/32 x quantities or
 * planes x H/4 workgroups; the PyTorch module issues ~100. */
int ffwm_guided_filter_forward(const void* x, const void* y, void* output, void* saved,
                               int64_t planes, int64_t H, int64_t W, int r, double eps, int dtype,
                               void* stream);

/* grad_x (OVERWRITTEN) of the above; y is data (the ground-truth image) and gets no gradient.
 * `workspace`: [2, planes, H, W] elements of the tensors' dtype, contents irrelevant on entry and exit. */
int ffwm_guided_filter_backward(const void* x, const void* y, const void* saved,
                                const void* grad_output, void* grad_x, void* workspace,
                                int64_t planes, int64_t H, int64_t W, int r, int dtype, void* stream);

/* The reference's whole contract (models/external_function.py:239-277): planes of any size (H, W <= 8192 and H W < 2^28, else
 * FFWM_ERR_SIZE), a guide of one channel broadcast over the channels of y, and the gradient for y.
 *   x [planes_x, H, W], y / output / grad_output [planes_y, H, W] with planes_y = planes_x * k: k = 1 is c_x == c_y, k = c_y is the
 *   one-channel guide (x plane p guides the y planes p k .. p k + k - 1, i.e. x [B,1,H,W] against y [B,C,H,W]).
 *   saved: 2 planes_x + 3 planes_y planes of H W elements: mean_x [planes_x], mean_y, A [planes_y], var_x+eps [planes_x], mean_A
 *   [planes_y] -- for k = 1 the [5, planes, H, W] of the entry points above, which may then be mixed with these.
 *   workspace: ffwm_guided_filter_workspace_bytes(planes_x, planes_y, H, W, dtype, backward) bytes (a negative ffwm_status for
 *   arguments the entry points refuse), contents irrelevant on entry and exit; 0 bytes (NULL allowed) for a forward call that the
 *   kernels above serve.
 *   backward: grad_x [planes_x, H, W] (summed over the k channels, channel 0 first) and grad_y [planes_y, H, W] are OVERWRITTEN;
 *   either may be NULL and is then neither computed nor written, but not both.
 * Calls that the four-launch kernels above serve (k = 1, H, W <= 128, no grad_y) run on them unchanged; everything else takes five
 * launches forward and four backward of wave-per-chunk sliding-window passes (csrc/guided_filter.hip, "the general path").
 * No atomics, no host synchronisation, bit-identical from run to run. */
int64_t ffwm_guided_filter_workspace_bytes(int64_t planes_x, int64_t planes_y, int64_t H, int64_t W,
                                           int dtype, int backward);
int ffwm_guided_filter_forward_general(const void* x, const void* y, void* output, void* saved,
                                       void* workspace, int64_t planes_x, int64_t planes_y, int64_t H,
                                       int64_t W, int r, double eps, int dtype, void* stream);
int ffwm_guided_filter_backward_general(const void* x, const void* y, const void* saved,
                                        const void* grad_output, void* grad_x, void* grad_y,
                                        void* workspace, int64_t planes_x, int64_t planes_y, int64_t H,
                                        int64_t W, int r, int dtype, void* stream);

/* ---- fused affine regularisation (FlowNet pre-training) -----------------------------------------
 * AffineRegularizationLoss.__call__ of models/losses.py:200-219 for one flow scale in ONE launch:
 *   loss_sum[0] += sum over b, both coordinate grids g = (flow + 1) / 2 * 128 and every kz x kz window p
 *                  of g of  p^T (K^T K) p            (the caller multiplies by loss_scale = 1 / (B h' w'))
 *   grad_flow  += d(loss_scale * that sum) / d flow   (may be NULL)
 * flow[B,2,h,w]; ktk[kz^2, kz^2] = the reference's `self.kernel` (K^T K, losses.py:192-198) in the
 * tensors' dtype; kernel_size in {3, 5, 7} (models/flownet_model.py:31).  The reference reaches the same
 * numbers through conv2d -> local_attn_reshape -> block_extractor -> avg_pool2d (those entry points remain;
 * ffwm_amd/losses.py composes them like the reference when `fused=False`). */
int ffwm_affine_regularization(const void* flow, const void* ktk, void* loss_sum, void* grad_flow,
                               int64_t B, int64_t h, int64_t w, int kernel_size, double loss_scale,
                               int dtype, void* stream);

/* ---- correlation column maximum (correctness loss of FlowNet pre-training) ----------------------
 * out[b, j] = max_i sum_k source[b, i, k] * target[b, k, j]   -- torch.max(torch.bmm(source_norm,
 * target_norm), dim=1)[0] of PerceptualCorrectness.calculate_loss (models/losses.py:347-353) without
 * the [B, N, N] matrix (1 GiB per sample at relu1_1), on fp32-in / fp32-accumulate MFMA.
 * source[B,N,C], target[B,C,N] contiguous float32, C in {64, 128, 256}, out[B,N]. */
int ffwm_correlation_colmax(const void* source, const void* target, void* out, int64_t B, int64_t N,
                            int64_t C, int dtype, void* stream);

/* The same maximum on the bf16 matrix instruction (v_mfma_f32_32x32x16_bf16, 16 x the fp32 MFMA rate), opt-in.  Every operand
 * element is split as hi = bf16_rn(x), lo = bf16_rn(x - hi); a product sum is lo.hi + hi.lo + hi.hi in one fp32 accumulator (lo.lo
 * dropped): three MFMAs per 16 k.  Operands, shapes, size limits, argument checks and error codes are those of
 * ffwm_correlation_colmax; profiler row `correlation_colmax_split` (the fp32 row's algorithmic bytes and flops).
 *   |prod_ij - ref_ij| <= (2^-16 + 3 C fp32 roundings) sum_k |s_ik t_kj|   (tests/colmax_split_bounds.py; 1-3e-6 on normalised
 *   features, the fp32 kernel: C roundings).  No atomics; two calls agree bit for bit.
 * Non-finite values: a NaN in source row i makes out[b, :] NaN, a NaN in target column j makes out[b, j] NaN alone; an INFINITE
 * operand has lo = NaN and so behaves as a NaN in its row / column (ffwm_correlation_colmax propagates the infinity instead);
 * finite |x| >= 2^127 may round to infinity and is outside the contract. */
int ffwm_correlation_colmax_split(const void* source, const void* target, void* out, int64_t B, int64_t N,
                                  int64_t C, int dtype, void* stream);

/* ---- fused sampling-correctness loss (FlowNet pre-training) -------------------------------------
 * PerceptualCorrectness.calculate_loss of models/losses.py:341-371 on its bilinear branch (:356-357), for one flow scale, after
 * the correlation maximum: grid_sample -> cosine_similarity -> exp -> mask -> sums, and the gradient for the flow, in ONE pass
 * over the channels (plus a one-block launch that adds the per-block sums in a fixed order).  Per pixel p = (b, y, x):
 *   the sampling position px = ((flow[b,0,p] + 1) Wi - 1) / 2, py likewise with Hi, and its four taps are those of
 *   ffwm_warp_forward (ATen grid_sampler_2d, bilinear / zeros / align_corners=False); an out-of-range tap counts as the value 0
 *   in the sample s_c and in its derivatives dx s_c = (1 - ty)(v01 - v00) + ty (v11 - v10), dy s_c likewise;
 *   D = sum_c s_c t_c, S = sum s_c^2, T = sum t_c^2, Px = sum t_c dx s_c, Qx = sum s_c dx s_c (Py, Qy likewise);
 *   ns = max(sqrt S, 1e-8), nt = max(sqrt T, 1e-8), cos = D / (ns nt)       (F.cosine_similarity: each norm clamped)
 *   m = exp(-cos / (corr_max[p] + eps))
 *   d m / d flow_x = -m / (corr_max[p] + eps) (Px / (ns nt) - [sqrt S > 1e-8] D Qx / (ns^3 nt)) Wi / 2     (y: Py, Qy, Hi / 2)
 * source[B,C,Hi,Wi], target[B,C,H,W], flow[B,2,H,W] (normalised absolute coordinates, ch0 = x), corr_max[B,H W],
 * mask[B,H W] or NULL (= all ones).  Outputs, all OVERWRITTEN with plain stores (one owner per pixel, no atomics):
 *   loss_map[B,H W] = m                              (NULL: not written)
 *   grad_flow[B,2,H,W] = mask d m / d flow           (NULL: not written); the caller scales it by grad_output / out[1]
 *   out[0] = (sum mask m - e1) / (sum mask + eps)    with a mask,    sum m / (B H W) - e1    without
 *   out[1] = sum mask + eps                          with a mask,    B H W                   without
 * e1 = exp(-1) rounded in the tensors' dtype, eps = the module's 1e-8.  The sums over the pixels are formed in double, per block
 * into `workspace` (ffwm_sampling_correctness_workspace_bytes(B, H, W, dtype) bytes, 8-byte aligned, contents irrelevant on entry
 * and exit; a negative ffwm_status for sizes the entry point refuses) and then in a fixed order: two calls agree bit for bit.
 * C >= 1 is arbitrary, Hi x Wi independent of H x W; a plane of 2^28 elements or more, or C Hi Wi elements of 4 GiB or more, is
 * FFWM_ERR_SIZE.  A non-finite flow samples nothing (m = 1, gradient 0) where the composition yields NaN: the entry point follows
 * the composition only where that is defined. */
int64_t ffwm_sampling_correctness_workspace_bytes(int64_t B, int64_t H, int64_t W, int dtype);
int ffwm_sampling_correctness(const void* source, const void* target, const void* flow, const void* corr_max,
                              const void* mask, void* loss_map, void* grad_flow, void* out, void* workspace,
                              int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, double e1,
                              double eps, int dtype, void* stream);

/* ---- fused landmark loss (FlowNet pre-training) ---------------------------------------------------
 * LandmarkLoss / MultiScaleLDLoss of models/losses.py:61-74,114-126 for ALL flow scales of one batch (1 <= n_scales <= 4) in one
 * call, with the gradient for every flow and WITHOUT float atomics (profiler rows `landmark_loss` and `landmark_loss_reduce`, a
 * one-block launch that adds the per-block sums in a fixed order).  Host arrays of n_scales entries: flows[i] -> [B,2,s_i,s_i],
 * grads (NULL, or grads[i] -> the same shape or NULL), sides[i] = s_i, divisors[i] = q_i >= 1, weights[i].  Device tensors:
 * lm_S, lm_F int64 [B,L,2] in (x, y) order, gate [B,L,2] in the flows' dtype, all contiguous.  Per scale, `div` rounding toward
 * minus infinity (torch.div(..., rounding_mode="floor")):
 *   (X, Y) = (lm_F[b,l,0] div q, lm_F[b,l,1] div q),    w_c = (lm_S[b,l,c] div q) * (2 / s) - 1
 *   e[b,l,c] = (flow[b,c,Y,X] - w_c) * gate[b,l,c],     mse = sum e^2 / (2 B L)
 *   out[1 + i] = mse_i,    out[0] = sum_i weights[i] * mse_i                                   (out: n_scales + 1 elements)
 *   grads[i][b,c,Y,X] = weights[i] / (B L) * sum over the landmarks of sample b on (X, Y) of gate^2 (flow - w_c); every other
 *   element is written as 0: the destination is OVERWRITTEN completely with plain stores (one owner per cell), no zero-fill.
 * A landmark with an lm_F component outside [0, s q) is never dereferenced: it adds 0 to the loss and the gradient of that scale
 * and still counts in the denominator.  *skipped (a device int32, overwritten) = the landmarks (b, l) that one scale or more
 * skipped.  lm_S is converted to the dtype before the product: exact below 2^24 (2^53).  Every sum meets in an order fixed by
 * the shapes (the loss in double, per block into `workspace`: ffwm_landmark_loss_workspace_bytes bytes, 8-byte aligned, contents
 * irrelevant on entry and exit; a negative ffwm_status for sizes the entry point refuses): two calls agree bit for bit.
 * Sides up to 4096 with s q < 2^31, B and L up to 2^30; beyond that FFWM_ERR_SIZE. */
int64_t ffwm_landmark_loss_workspace_bytes(const int64_t* sides, int n_scales, int64_t B, int64_t L, int dtype);
int ffwm_landmark_loss(const void* const* flows, void* const* grads, const int64_t* sides, const int64_t* divisors,
                       const double* weights, int n_scales, const void* lm_S, const void* lm_F, const void* gate,
                       void* out, void* skipped, void* workspace, int64_t B, int64_t L, int dtype, void* stream);

/* Fused extractor + attention consumer (the GFLA-style local attention the cfg-5 shape
 * models): what the reference API can only express as
 *     avg_pool2d(BlockExtractor(source, flow, k) * LocalAttnReshape(weights, k), k, k)
 * (models/external_function.py:14-101 + F.avg_pool2d, the same composition models/losses.py:211-219 uses),
 * without the k^2-fold expanded tensors:
 *     out[b,c,y,x] = (sum_ij sample_ij(b,c,y,x) * weights[b, i*k + j, y, x]) / k^2,
 * sample_ij = the block_extractor value at (y*k + i, x*k + j).  Products and the row-major sum are rounded
 * separately and divided once, like the three ATen/extension kernels of the composition.
 * source[B,C,Hs,Ws], flow_field[>=B,2,Hf,Wf], weights[B,k*k,Hf,Wf], output[B,C,Hf,Wf] (overwritten). */
int ffwm_block_attention_forward(const void* source, const void* flow_field, const void* weights, void* output,
                                 int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf,
                                 int kernel_size, int dtype, void* stream);

/* grad_source[B,C,Hs,Ws] +=, grad_flow_field[B,2,Hf,Wf] +=, grad_weights[B,k*k,Hf,Wf] += for
 * grad_output[B,C,Hf,Wf]; any of the three may be NULL.  The extractor's grad_output window is
 * (grad_output / k^2) * weights_ij -- a channel-independent window times one number per channel, so (round 6) grad_source comes from
 * per-pixel cell coefficients Wy^T w Wx scaled per channel, grad_flow_field and grad_weights from P = sum_c (g_c / k^2) S_c over the
 * (k+1)^2 source neighbourhood: two launches for fp32 / k = 3 with grad_source wanted (csrc/block_extractor.hip: ba_bwd_src_kernel,
 * ba_bwd_pix_kernel), the per-element kernel otherwise. */
int ffwm_block_attention_backward(const void* source, const void* flow_field, const void* weights,
                                  const void* grad_output, void* grad_source, void* grad_flow_field,
                                  void* grad_weights, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf,
                                  int64_t Wf, int kernel_size, int dtype, void* stream);

/* Weight (and bias) gradient of a 3x3 / stride 1 / pad 1 / dilation 1 / groups 1 convolution (the layer type of
 * the FFWM and FlowNet conv stacks, models/base_networks.py:59-165,274-347; the grad_weight / grad_bias outputs of
 * ATen's convolution_backward) on fp32-in / fp32-accumulate MFMA, NCHW, no transposes:
 *     grad_weight[K,C,3,3][k,c,r,s] += sum_{b,y,x} grad_output[b,k,y,x] * input[b,c,y+r-1,x+s-1]
 *     grad_bias[K][k]               += sum_{b,y,x} grad_output[b,k,y,x]        (NULL: skipped)
 * input[B,C,H,W], grad_output[B,K,H,W] contiguous float32, W a multiple of 64; the caller zero-fills
 * grad_weight and grad_bias (pixel slices are combined with atomics). */
int ffwm_conv3x3_wgrad(const void* input, const void* grad_output, void* grad_weight, void* grad_bias, int64_t B,
                       int64_t C, int64_t K, int64_t H, int64_t W, int dtype, void* stream);

/* The same, restricted to the block grad_weight[k_begin:k_end, c_begin:c_end] and grad_bias[k_begin:k_end] (tensor
 * extents and strides are still K and C). */
int ffwm_conv3x3_wgrad_block(const void* input, const void* grad_output, void* grad_weight, void* grad_bias, int64_t B,
                             int64_t C, int64_t K, int64_t H, int64_t W, int64_t k_begin, int64_t k_end, int64_t c_begin,
                             int64_t c_end, int dtype, void* stream);

/* Training-mode BatchNorm2d fused with the LeakyReLU that follows it (the conv blocks of
 * models/base_networks.py:12-31,207-264,381-413): y = leaky_relu(F.batch_norm(x, running_mean, running_var, weight,
 * bias, training=True, momentum, eps), negative_slope).  x, y [B,C,H,W] contiguous float32 (16-byte aligned),
 * HW = H*W; weight / bias [C] or NULL; running_mean / running_var [C] updated in place (both NULL: not tracked);
 * save_mean / save_invstd [C] are written for the backward pass.  scratch: NULL, or 2*C + (C+1)/2 ZERO-FILLED doubles (two sums
 * per channel, then one 32-bit arrival counter per channel) -- with it a channel with few workgroups' worth of parallelism
 * (C < 1024) is split over several workgroups (two launches).  The kernels leave the scratch ZERO-FILLED again (the last
 * workgroup of a channel to read the sums clears them): one buffer serves every later call on the same stream. */
int ffwm_bn_lrelu_forward(const void* x, const void* weight, const void* bias, void* running_mean, void* running_var,
                          void* y, void* save_mean, void* save_invstd, void* scratch, int64_t B, int64_t C, int64_t HW,
                          double eps, double momentum, double negative_slope, int dtype, void* stream);

/* grad_x [B,C,H,W], grad_weight [C], grad_bias [C] are OVERWRITTEN (each channel is produced by one workgroup); any
 * of them may be NULL.  The activation mask is recomputed from x, the forward output is not needed. */
int ffwm_bn_lrelu_backward(const void* x, const void* grad_out, const void* weight, const void* bias,
                           const void* save_mean, const void* save_invstd, void* grad_x, void* grad_weight,
                           void* grad_bias, void* scratch, int64_t B, int64_t C, int64_t HW, double negative_slope,
                           int dtype, void* stream);

/* The tail of a residual block, activ(blocks(x) + input(x)) with blocks ending in a training-mode BatchNorm2d and input = a 1x1
 * convolution (models/base_networks.py:207-233), as one kernel per direction: y = act(BatchNorm(x) + res + rbias[c]) where res is the
 * shortcut convolution's output WITHOUT its bias and rbias that bias (NULL: none); act 0 = LeakyReLU(negative_slope), 1 = sigmoid.
 * Statistics, running buffers, save_mean / save_invstd and scratch as in ffwm_bn_lrelu_forward.  Replaces, per block and direction,
 * the library's BatchNorm kernel, the GEMM path's separate bias add and the add + activation pass. */
int ffwm_bn_res_act_forward(const void* x, const void* weight, const void* bias, void* running_mean, void* running_var,
                            const void* res, const void* rbias, void* y, void* save_mean, void* save_invstd, void* scratch,
                            int64_t B, int64_t C, int64_t HW, double eps, double momentum, double negative_slope, int act,
                            int dtype, void* stream);
/* grad_res = grad_out * act'(.) (taken from the saved output y; also the gradient of `input(x)`), grad_x = BatchNorm backward of
 * it, grad_weight / grad_bias = the BatchNorm's affine gradients (grad_bias is the gradient of rbias too).  grad_x, grad_res,
 * grad_weight, grad_bias may be NULL. */
int ffwm_bn_res_act_backward(const void* x, const void* y, const void* grad_out, const void* weight, const void* save_mean,
                             const void* save_invstd, void* grad_x, void* grad_res, void* grad_weight, void* grad_bias,
                             void* scratch, int64_t B, int64_t C, int64_t HW, double negative_slope, int act, int dtype,
                             void* stream);

/* LightCNN's max-feature-map activation (lightcnn/light_cnn.py `mfm.forward`: torch.split + torch.max):
 * y[B,C,HW] = max(x[B,0:C,HW] + bias[0:C], x[B,C:2C,HW] + bias[C:2C]); bias [2C] or NULL (the bias of the layer in front,
 * folded in: bit-identical to adding it first); backward grad_x[B,2C,HW] (overwritten) with ATen's tie rule for
 * `maximum` (equal halves share the gradient).  Contiguous float32. */
int ffwm_mfm_forward(const void* x, const void* bias, void* y, int64_t B, int64_t C, int64_t HW, int dtype, void* stream);
int ffwm_mfm_backward(const void* x, const void* bias, const void* grad_y, void* grad_x, int64_t B, int64_t C, int64_t HW,
                      int dtype, void* stream);

/* ---- residual-block tails and the warp-attention gate of netG (models/base_networks.py:207-233, 326-333) ----------------
 * ResidualBlock.forward = activ(blocks(x) + input(x)) and FFWM.forward's `skip = skip * att_i(skip)` (att_i ends in a sigmoid
 * ResidualBlock) as one pass each instead of 2-3 element-wise launches.  Contiguous float32, n elements, 16-byte aligned.
 *   ffwm_add_act_forward:       y = act(a + b), act 1 = LeakyReLU(negative_slope > 0), 3 = sigmoid (y may alias a or b)
 *   ffwm_add_act_backward:      grad_z = grad_y * act'(a + b), formed from y alone (grad_z may alias grad_y); it is the gradient of
 *                               a AND of b
 *   ffwm_sigmoid_gate_forward:  att = sigmoid(a + b), y = x * att
 *   ffwm_sigmoid_gate_backward: grad_z = grad_y * x * att * (1 - att) (gradient of a and of b), grad_x = grad_y * att
 * ATen's operation order throughout (results equal the PyTorch composition's bit for bit up to expf). */
int ffwm_add_act_forward(const void* a, const void* b, void* y, int64_t n, int act, double negative_slope, int dtype, void* stream);
int ffwm_add_act_backward(const void* y, const void* grad_y, void* grad_z, int64_t n, int act, double negative_slope, int dtype,
                          void* stream);
int ffwm_sigmoid_gate_forward(const void* a, const void* b, const void* x, void* att, void* y, int64_t n, int dtype, void* stream);
int ffwm_sigmoid_gate_backward(const void* x, const void* att, const void* grad_y, void* grad_z, void* grad_x, int64_t n, int dtype,
                               void* stream);

/* y[B,C,HW] = relu(h[B,C,HW] + bias[C]) -- the bias add and ReLU behind the frozen VGG19 convs (models/losses.py:398-519)
 * as one pass; y may alias h. */
int ffwm_bias_relu_forward(const void* h, const void* bias, void* y, int64_t B, int64_t C, int64_t HW, int dtype, void* stream);

/* ---- FlowNet eval forward (models/base_networks.py:59-165, BASELINE configs[1]): the layers around the dense convolutions
 * once BatchNorm is folded into the conv weights (ffwm_amd/flownet_eval.py).  Contiguous float32.
 *
 * ffwm_bias_act_forward: y = act(h[B,C,HW] + bias[C]) (bias may be NULL); act 0 = none, 1 = LeakyReLU(negative_slope),
 * 2 = tanh.  Two optional destinations (either may be NULL, y may alias h): channel c of sample b is written at
 * y + b * y_batch_stride + c * HW, so a destination can be a channel slice of a wider concatenation buffer
 * (torch.cat of base_networks.py:133-151 without its copy kernel). */
int ffwm_bias_act_forward(const void* h, const void* bias, void* y, void* y2, int64_t B, int64_t C, int64_t HW,
                          int64_t y_batch_stride, int64_t y2_batch_stride, int act, double negative_slope, int dtype,
                          void* stream);
/* FlowNet's thin-channel full-resolution 3 x 3 layers (models/base_networks.py:64-112: conv0 6 -> 64, inter_conv0 18 -> 16) by a direct
 * kernel: a lane owns one pixel and 8 / 16 output channels, weights as scalar operands.  weight_ctk = the layer's weights re-arranged by
 * the host from Conv2d's [K][C][3][3] to [C][3][3][K]; K % 8 == 0.  Conv2d(C, K, 3, 1, 1) -> y[B,K,H,W] contiguous; act = 1:
 * LeakyReLU(negative_slope) after the bias (bias may be NULL).  fp32. */
int ffwm_conv_thin_forward(const void* x, const void* weight_ctk, const void* bias, void* y, int64_t B, int64_t C, int64_t H, int64_t W,
                           int64_t K, int act, double negative_slope, int dtype, void* stream);

/* predict_flow* (base_networks.py:45-49): y[B,2,H,W] = tanh(conv2d(x[B,C,H,W], weight[2,C,3,3], bias[2], stride 1, pad 1)) */
int ffwm_flow_head_forward(const void* x, const void* weight, const void* bias, void* y, int64_t B, int64_t C, int64_t H,
                           int64_t W, int dtype, void* stream);
/* upsampled_flow*_to_* (base_networks.py:104-109): out = conv_transpose2d(flow[B,2,H,W], weight[2,2,4,4], bias[2], stride 2,
 * pad 1) -> [B,2,2H,2W], sample b written at out + b * out_batch_stride (a channel slice of the concatenation buffer). */
int ffwm_flow_up_forward(const void* flow, const void* weight, const void* bias, void* out, int64_t B, int64_t H, int64_t W,
                         int64_t out_batch_stride, int dtype, void* stream);

/* Training: the backward of the two launch-lean layers above (models/base_networks.py:45-49,104-109).
 * ffwm_flow_head_backward: y = the head's output, grad_y [B, 2, H, W] contiguous; writes grad_z = grad_y * (1 - y^2) [B, 2, H, W] (the
 * row operand of the weight gradient, ffwm_conv2d_wgrad_tiled(grad_z, x, ...), whose fused row sum is the bias gradient) and
 * grad_x [B, C, H, W].  ffwm_flow_up_backward: grad_x [B, 2, H, W] from grad_out [B, 2, 2H, 2W] read with its batch stride (a
 * channel slice of the decoder concatenation's gradient needs no copy). */
int ffwm_flow_head_backward(const void* y, const void* grad_y, const void* weight, void* grad_z, void* grad_x, int64_t B, int64_t C,
                            int64_t H, int64_t W, int dtype, void* stream);
int ffwm_flow_up_backward(const void* grad_out, const void* weight, void* grad_x, int64_t B, int64_t H, int64_t W,
                          int64_t grad_out_batch_stride, int dtype, void* stream);

/* fp32 MFMA implicit-GEMM convolution forward, NCHW, for the layers the vendor library wraps in layout transposes:
 * nn.Conv2d(C, K, kernel 3 or 4, stride 1 or 2, pad) or -- transposed == 1 -- nn.ConvTranspose2d(C, K, 4, 2, 1)
 * (weight [C, K, 4, 4]) of models/base_networks.py:12-31,64-112; transposed == 2 / 3: the data gradient of Conv2d(3, 2, 1) /
 * Conv2d(3, 1, 1) with `input` = grad_output and the layer's own weight tensor.  output sample b starts at
 * output + b * out_batch_stride (a channel slice of a concatenation buffer is a valid destination); output2 (NULL: none) is a
 * second destination that receives the same values (the decoder's concatenation slice next to the skip tensor).  act: 0 none,
 * 1 LeakyReLU(negative_slope), 2 tanh, applied after the bias.  Exact fp32 (v_mfma_f32_32x32x2_f32).
 * workspace (ABI 5; NULL: never split): a layer with so few output pixels that its tiles do not fill the chip is cut along its
 * REDUCTION when `workspace_bytes >= ffwm_conv2d_forward_workspace(...)` (16-byte aligned, contents irrelevant, nothing to
 * zero-fill): every slice stores its partial sums into its own slot and a second launch adds the slots in slice order and
 * applies bias / activation -- no float atomics, so the output is bit-reproducible.  (ABI <= 4 added the slices atomically into
 * a caller-zeroed output and left bias / activation to ffwm_bias_act_forward.) */
int64_t ffwm_conv2d_forward_workspace(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int kernel, int stride, int pad,
                                      int transposed);
int ffwm_conv2d_forward(const void* input, const void* weight, const void* bias, void* output, void* output2, int64_t B, int64_t C,
                        int64_t H, int64_t W, int64_t K, int kernel, int stride, int pad, int transposed, int64_t out_batch_stride,
                        int64_t out2_batch_stride, int act, double negative_slope, void* workspace, int64_t workspace_bytes,
                        int dtype, void* stream);

/* fp32 MFMA weight gradient of the convolutions ffwm_conv2d_forward serves, one launch, no layout transposes:
 *   grad_weight[k][(c, r, s)] += sum_{b, oy, ox} rows[b, k, oy, ox] * gathered[b, c, oy * stride + r - pad, ox * stride + s - pad]
 * nn.Conv2d(C, K, kernel, stride, pad):   rows = grad_output [B,K,Ho,Wo], gathered = input [B,C,H,W]         -> [K, C, k, k]
 * nn.ConvTranspose2d(Ci, Co, 4, 2, 1):    rows = input [B,Ci,H,W],        gathered = grad_output [B,Co,2H,2W] -> [Ci, Co, 4, 4]
 * (kernel = 4, stride = 2, pad = 1).  grad_weight must be ZERO-FILLED (or hold the value to accumulate into): the pixel
 * slices of the reduction are added atomically. */
int ffwm_conv2d_wgrad(const void* rows, const void* gathered, void* grad_weight, int64_t B, int64_t K, int64_t Ho, int64_t Wo,
                      int64_t C, int64_t H, int64_t W, int kernel, int stride, int pad, int dtype, void* stream);

/* The same weight gradient on the tiled kernel (128 x 128 tiles of grad_weight, pixels linearised over the batch, one barrier per
 * 32 pixels; csrc/conv_bwd.hip "tiled variant"): grad_weight is OVERWRITTEN -- the library zero-fills it itself when the pixel
 * range is cut into slices that meet by atomics -- and grad_bias[K] (NULL: not wanted; Conv2d only: the sum of `rows` over batch
 * and pixels = convolution_backward's grad_bias) comes out of the same pass.  Needs Ho * Wo % 4 == 0 and a 16-byte aligned `rows`
 * (status FFWM_ERR_ARG otherwise: use ffwm_conv2d_wgrad).  prezeroed != 0 (ABI 5): grad_weight / grad_bias arrive ZEROED (slices of a gradient
 * arena cleared by one launch per step) and a sliced launch skips its own zero-fill -- an argument since ABI 5, the process-global
 * option of ABI 4 was not thread-safe. */
int ffwm_conv2d_wgrad_tiled(const void* rows, const void* gathered, void* grad_weight, void* grad_bias, int64_t B, int64_t K,
                            int64_t Ho, int64_t Wo, int64_t C, int64_t H, int64_t W, int kernel, int stride, int pad, int prezeroed,
                            int dtype, void* stream);

/* 3x3 / stride 1 / pad 1 convolution by Winograd F(2x2, 3x3) on the fp32 MFMA units (csrc/conv_winograd.hip): the
 * forward (data_gradient = 0: weight [K, C, 3, 3]) or the data gradient (data_gradient = 1: input = grad_output with C =
 * the layer's OUTPUT channels, K = its input channels, weight = the layer's own [C, K, 3, 3]) of Conv2d(.., 3, 1, 1)
 * (models/base_networks.py:207-233: the residual blocks of netG; :59-112 FlowNet's conv*_1 / inter_conv*).
 * output [B, K, H, W] = conv + bias (NULL: none), then LeakyReLU(slope) when act = 1 (slope 0: ReLU).  workspace: device
 * memory of ffwm_conv3x3_winograd_workspace_bytes(K, C) bytes (the transformed weights; rewritten by every call).
 * data_gradient + 2: the workspace still holds the transformed weights of an earlier call with the same weight values,
 * direction, K, C and (W % 4 == 0) -- frozen networks (VGG19, LightCNN: models/losses.py:398-519) skip the transform. */
int64_t ffwm_conv3x3_winograd_workspace_bytes(int64_t K, int64_t C);
/* In how many pieces ffwm_conv3x3_winograd_forward will cut the reduction (input channels) of this call: 1, 2 or 4.  A call whose
 * (64 tiles, 64 output channels) pairs fill less than half the CUs (256 -> 256 at 32 x 32, batch 8) is cut so that one round of
 * persistent workgroups covers the chip; the pieces' partial outputs meet by atomics in the output, which the library zero-fills
 * itself.  Only for act = 0.  The caller's routing policy (ffwm_amd/conv.py) uses it to price a call. */
int ffwm_conv3x3_winograd_splits(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int act);

/* The weight transforms of several Winograd calls in ONE launch.  Item i fills `workspace` (ffwm_conv3x3_winograd_workspace_bytes(K, C)
 * bytes) exactly as ffwm_conv3x3_winograd_forward(.., K, C, data_gradient, ..) would for an input whose width is (or is not) a
 * multiple of 4; that call is then made with data_gradient + 2 (reuse).  K / C in the CALL's terms: for the data gradient K = the
 * layer's input channels, C = its output channels, weight = the layer's own [C, K, 3, 3].  (ffwm_amd/spectral_norm.py: all layers of
 * a spectrally normalised network right after its batched normalisation.) */
typedef struct ffwm_wino_weights {
    const void* weight;
    void* workspace;
    int64_t K, C;
    int data_gradient;            /* 0 = forward, 1 = data gradient */
    int width_multiple_of_4;      /* of the planes the transform will be used on (selects the thin-tail split of K) */
} ffwm_wino_weights;
int ffwm_conv3x3_winograd_weights_multi(const ffwm_wino_weights* items, int n, int dtype, void* stream);
int ffwm_conv3x3_winograd_forward(const void* input, const void* weight, const void* bias, void* output, void* workspace,
                                  int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int data_gradient, int act,
                                  double slope, int dtype, void* stream);

/* The same convolution in the classic three-launch form, for FROZEN layers on small planes (csrc/conv_winograd_gemm.hip): input
 * transform, 16 independent fp32 MFMA GEMMs M_p = U_p V_p (one per Winograd position), output transform.  No atomics, no split of
 * the reduction: deterministic.  float32 only.
 *   ffwm_conv3x3_wg_weights: weight -> U = G w G^T, ffwm_conv3x3_wg_weights_bytes(K, C) bytes, stored [16][Cp / 4][K][4]
 *     (Cp = C rounded up to 16, four input channels interleaved, channels past C zero).  K / C in the CALL's terms: data_gradient = 1 takes the layer's own
 *     [C, K, 3, 3] transposed and rotated.  Made once per layer and direction; the forward call only reads it.
 *   ffwm_conv3x3_wg_forward: input [B, C, H, W] -> output [B, K, H, W] (epilogue FFWM_WG_MFM: [B, K / 2, H, W], K even).
 *     bias [K] or NULL (FFWM_WG_NONE ignores it).  relu_mask or NULL: a tensor of the input's shape; the input transform reads
 *     input * (relu_mask > 0) as ATen's threshold_backward selects it (mask <= 0 -> 0, else the input: a NaN mask passes it) --
 *     the data gradient behind a ReLU without the separate masking pass.  workspace: ffwm_conv3x3_wg_workspace_bytes(B, C, H, W, K)
 *     bytes, 16-byte aligned, rewritten by every call (V and M).
 *   ffwm_conv3x3_wg_tile: the GEMM tile (64 or 128) the plan of that call takes: 128 x 128 when that still gives every compute
 *     unit a workgroup, else 64 x 64 (0 for a non-positive size).
 *   ffwm_conv3x3_wg_forward_tiled: the same call with the GEMM tile fixed (tile = 64 or 128; 0 = the plan's): for tests and
 *     measurements. */
enum { FFWM_WG_NONE = 0, FFWM_WG_BIAS = 1, FFWM_WG_BIAS_RELU = 2, FFWM_WG_BIAS_MFM = 3 };
int64_t ffwm_conv3x3_wg_weights_bytes(int64_t K, int64_t C);
int64_t ffwm_conv3x3_wg_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K);
int ffwm_conv3x3_wg_weights(const void* weight, void* U, int64_t K, int64_t C, int data_gradient, int dtype, void* stream);
int ffwm_conv3x3_wg_forward(const void* input, const void* U, const void* bias, void* output, void* workspace,
                            int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, const void* relu_mask,
                            int dtype, void* stream);
int ffwm_conv3x3_wg_tile(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K);
int ffwm_conv3x3_wg_forward_tiled(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                  int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, const void* relu_mask,
                                  int tile, int dtype, void* stream);

/* The forward of the same three-launch route with its 16 GEMMs on the bf16 matrix instruction (csrc/conv_winograd_gemm_split.hip):
 * float32 tensors in and out; U = G w G^T and V = B^T d B are computed in fp32 as above, every entry x is then split in two bf16
 * terms, hi = bf16_rn(x), lo = bf16_rn(x - hi), and a product sum is taken as sum_c (U_lo V_hi + U_hi V_lo + U_hi V_hi) in one fp32
 * accumulator (v_mfma_f32_32x32x16_bf16, three per 16 channels).  No atomics, no split of the reduction: deterministic.  Forward
 * only, no ReLU mask, no max-feature-map.
 *   Error per output element against the float64 convolution of the given tensors, u = 2^-24, MAG = 1 + 2^-6, mag_patch = sum_c (max
 *   |x_c| over the 4 x 4 patch of the element's 2 x 2 tile) (sum of |w_kc| over the 9 taps) + |bias_k|:
 *       |y - ref| <= 16 (2^-16 MAG + 4 (3 C + 11) u MAG) mag_patch + (4 + post) u |ref| + eta
 *   (post = 1 behind LeakyReLU; eta ~ 1e-36 covers bf16 terms, products and partial sums below 2^-126 that may be flushed to zero;
 *   derivation: tests/wino_split_cases.py).  At C = 64 that is 1.0e-3 mag_patch against 2.9e-4 of the fp32 route's bound.
 *   Non-finite contract: a NaN in the input makes the outputs inside the reach of its 4 x 4 patches NaN, a NaN in a weight its output
 *   channel.  An INFINITE entry of U or V has hi = inf and lo = bf16(inf - inf) = NaN, so an infinity in the input or a weight
 *   behaves as such a NaN.  Finite |x| >= 2^125 is outside the contract: V sums four inputs, and hi may round to infinity.
 *   ffwm_conv3x3_wg_split_weights: weight [K, C, 3, 3] -> the split U, ffwm_conv3x3_wg_split_weights_bytes(K, C) bytes, 16-byte
 *     aligned, stored [16][Cp / 8][hi, lo][K][8] bf16 (Cp = C rounded up to 32, channels past C zero).  Made once per layer.
 *   ffwm_conv3x3_wg_split_forward: input [B, C, H, W] -> output [B, K, H, W].  bias [K] (NULL with FFWM_WGS_NONE).  workspace:
 *     ffwm_conv3x3_wg_split_workspace_bytes(B, C, H, W, K) bytes (enough for either tile), 16-byte aligned, rewritten by every call.
 *     tile: 64 or 128 fixes the GEMM tile, 0 takes the plan's (ffwm_conv3x3_wg_split_tile: the rule of ffwm_conv3x3_wg_tile). */
enum { FFWM_WGS_NONE = 0, FFWM_WGS_BIAS = 1, FFWM_WGS_BIAS_LRELU = 2 };
int64_t ffwm_conv3x3_wg_split_weights_bytes(int64_t K, int64_t C);
int64_t ffwm_conv3x3_wg_split_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K);
int ffwm_conv3x3_wg_split_weights(const void* weight, void* U, int64_t K, int64_t C, int dtype, void* stream);
int ffwm_conv3x3_wg_split_tile(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K);
int ffwm_conv3x3_wg_split_forward(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                  int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, double negative_slope,
                                  int tile, int dtype, void* stream);
/* The same GEMM for the FROZEN loss networks of the train step (VGG19, LightCNN under autograd; loss_precision="bf16x3"): the data
 * gradient with its ReLU mask and the epilogues of the fp32 route.  Bounds: tests/wino_split_train_cases.py.
 *   ffwm_conv3x3_wg_split_weights_dgrad: the layer's own weight [K, C, 3, 3], read transposed and rotated by 180 degrees -> the
 *     split U of the data gradient (C output rows, reduction over K rounded up to 32), ffwm_conv3x3_wg_split_weights_bytes(C, K)
 *     bytes: bit for bit ffwm_conv3x3_wg_split_weights of weight.transpose(0, 1).flip(2, 3).
 *   ffwm_conv3x3_wg_split_apply: ffwm_conv3x3_wg_split_forward with the epilogue codes FFWM_WG_* (ReLU by torch.relu's rule: NaN
 *     stays NaN, -inf gives 0; max-feature-map: maximum(a, b) with ATen's NaN rule of rows k and k + K / 2, output [B, K / 2, H, W],
 *     K even) and relu_mask (NULL, or a tensor of the input's shape: the input is read as `mask <= 0 ? 0 : x`, so a NaN in the mask
 *     lets the value pass and a masked-out infinity or NaN is a zero).  Workspace, plan and tile as ffwm_conv3x3_wg_split_forward. */
int ffwm_conv3x3_wg_split_weights_dgrad(const void* weight, void* U, int64_t K, int64_t C, int dtype, void* stream);
int ffwm_conv3x3_wg_split_apply(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, const void* relu_mask,
                                int tile, int dtype, void* stream);

/* One Adam step (no weight decay, no amsgrad: torch.optim.Adam as models/ffwm_model.py:46-49 and
 * models/flownet_model.py:33 construct it) over FLAT float32 arrays of n elements, 16-byte aligned: parameters,
 * gradients, first and second moments.  `step` is the 1-based step count (bias corrections 1 - beta^step). */
int ffwm_adam_step(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, int64_t n, double lr,
                   double beta1, double beta2, double eps, int64_t step, int dtype, void* stream);

/* The same step with the step counter in DEVICE memory (a step inside a captured hipGraph: a replay runs no host code).  state:
 * FOUR doubles (ABI 3; three before): state[0] = steps taken so far (start it at 0), state[1] and state[2] are scratch,
 * state[3] = learning-rate override -- when >= 0 it replaces `lr`, so that a learning-rate schedule reaches a captured step
 * (`lr` is baked into the graph as a kernel argument; the host writes state[3] between replays); start it at a NEGATIVE value for
 * "no override" (ABI 4; ABI 3 took 0 for "none", so a schedule that reached 0.0 could not freeze the weights).  Two launches. */
int ffwm_adam_step_device(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, int64_t n, double lr, double beta1,
                          double beta2, double eps, void* state, int dtype, void* stream);

/* ---- gradient health (csrc/grad_health.hip) and the Adam step it guards (csrc/adam.hip) ---------------------------------------
 * What torch.nn.utils.clip_grad_norm_ and an `if not torch.isfinite(norm)` in front of optimizer.step() do in an eager loop, with
 * the numbers and the decision in DEVICE memory, so that both can sit inside a captured step (a replay runs no host code).
 *
 * ffwm_grad_health: grads = n float32 values, 16-byte aligned, READ ONLY.  seg_end = n_seg ascending ends in elements, read from
 * DEVICE memory; at most FFWM_GRAD_HEALTH_MAX_SEGMENTS; the last end is n; every end but the last is a multiple of 4 (a segment starts
 * on a 16-byte boundary, as every parameter of the reducer's flat array does).  record = 4 * n_seg DEVICE doubles, 16-byte aligned:
 * for segment s, over its FINITE elements, record[4 s] = sum g^2 and record[4 s + 1] = max |g|; record[4 s + 2] = the count of its
 * non-finite elements (NaN, +inf, -inf), record[4 s + 3] = its element count.  An empty segment, or one without a finite element,
 * gives a sum of 0 and a maximum of 0.  Squares and sums are double (1e-30, 1e25 and denormals count with their value).
 * No atomics: a chunk pass writes one partial per FFWM_GRAD_HEALTH_CHUNK elements of a segment (counted from the segment's start) into
 * `workspace` (16-byte aligned, at least ffwm_grad_health_workspace_bytes(n, n_seg) bytes; 0 for arguments the call would refuse), a
 * second pass adds a segment's partials; csrc/grad_health.hip states the order of every sum.  The result is a function of the values
 * and the table alone: two calls agree bit for bit, whatever the grid.  Only `workspace` and `record` are written.
 * Refused with FFWM_ERR_ARG: NULL or misaligned pointers, n < 1, n_seg outside 1 .. 16, a workspace that is too small, and a table that
 * is not as stated.  The table is in device memory: on a stream that is NOT being captured the call copies its 8 * n_seg bytes back and
 * waits for the stream -- the one entry point that does -- to check it; on a stream that is being captured it cannot, and the kernels
 * read the table through a clamp (every end into [previous end, n], rounded down to a multiple of 4, the last end n), so that no
 * table makes a load leave the array.  Two launches, safe to capture. */
#define FFWM_GRAD_HEALTH_CHUNK 8192
#define FFWM_GRAD_HEALTH_MAX_SEGMENTS 16
int ffwm_grad_health(const void* grads, int64_t n, const int64_t* seg_end, int n_seg, void* workspace, size_t workspace_bytes,
                     void* record, int dtype, void* stream);
size_t ffwm_grad_health_workspace_bytes(int64_t n, int n_seg);

/* ffwm_adam_step_device behind a guard.  `state` = its 4 doubles with the same meaning (the learning-rate override included).
 * `record` = what ffwm_grad_health wrote for this range (4 * n_seg doubles).  `guard` = 6 DEVICE doubles, zero at the start:
 *     guard[0] skip flag of this call        guard[1] scale of this call (a float value; 0 for a skipped call)
 *     guard[2] steps skipped so far          guard[3] steps seen so far
 *     guard[4] total sum g^2 of this call    guard[5] total non-finite count of this call
 * A one-thread kernel adds the segments' sums in segment order and decides:
 *   skip       skip_nonfinite != 0 and the non-finite count > 0: flag = 1, skipped += 1, state[0..2] untouched (the bias corrections
 *              do not move); the streaming kernel reads the flag and returns: params, exp_avg, exp_avg_sq stay bit for bit.
 *   otherwise  the state advances exactly as in ffwm_adam_step_device; scale = 1 when max_norm <= 0, else
 *              min(1, max_norm / (sqrt(total) + 1e-6)) computed in double and rounded once to float -- the coefficient of
 *              torch.nn.utils.clip_grad_norm_.  The streaming kernel multiplies each gradient by the float scale in registers (the
 *              gradient array is not written) and takes the step: with a scale of exactly 1 the result equals
 *              ffwm_adam_step_device's bit for bit.
 * max_norm > 0 with skip_nonfinite == 0 is refused with FFWM_ERR_ARG (a clip over a non-finite norm has no meaning).
 * The guard protects params and both moments; whatever the forward pass of the bad step already wrote (BatchNorm running statistics)
 * is not restored.  Two launches, safe to capture. */
int ffwm_adam_step_guarded(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, int64_t n, double lr, double beta1,
                           double beta2, double eps, void* state, const void* record, int n_seg, double max_norm, int skip_nonfinite,
                           void* guard, int dtype, void* stream);

/* One SGD-momentum step (torch.optim.SGD with dampening 0 and no Nesterov, as lightcnn/finetune.py:88-90 constructs it) over FLAT
 * float32 arrays of n elements, 16-byte aligned: parameters, gradients and the momentum buffer (start it at zero: that is torch's
 * first step).  Element i belongs to segment s, the first one with seg_end[s] > i (DEVICE int64, ascending, seg_end[n_seg - 1] == n,
 * n_seg <= 1024), and takes the learning rate and the weight decay of group seg_group[s] (DEVICE int32) from group_lr / group_wd
 * (DEVICE doubles, n_groups <= 16, rounded to float32; a group index outside the table is clamped into it):
 *     g' = g + wd p,    buf = momentum buf + g',    p = p - lr buf      (the last line one fma: five roundings per element)
 * Everything a schedule changes lives in device memory, so the next replay of a captured step sees it.  One launch. */
int ffwm_sgd_step(void* params, const void* grads, void* momentum_buf, int64_t n, const int64_t* seg_end, const int32_t* seg_group,
                  int n_seg, const double* group_lr, const double* group_wd, int n_groups, double momentum, int dtype, void* stream);

/* ---- classifier loss of LightCNN fine-tuning (csrc/softmax_xent.hip; lightcnn/finetune.py:109,152-159,294-307) ---------------
 * nn.CrossEntropyLoss (mean) over logits [B, N], its gradient, and accuracy(output, target, (1, 5)), in three launches without
 * float atomics; float32 and float64.  target: DEVICE int64 [B].
 *   row_loss[b] = logsumexp(x_b) - x_b[t_b]      (the row maximum subtracted; NULL: not written)
 *   rank[b]     = #{j : x_bj > x_bt} + #{j < t : x_bj == x_bt}    (int32, NULL: not written; ties go to the lower index, a NaN ranks
 *                 above everything and equal to another NaN: ffwm_cosine_topk's rule)
 *   grad_logits[b, j] = (softmax(x_b)[j] - [j == t_b]) / B        (NULL: not written; else OVERWRITTEN completely)
 *   out[0] = mean of row_loss,  out[1] / out[2] = 100 #{b : rank[b] < 1 / 5} / B
 * A NaN logit makes its row's loss and gradient NaN, and out[0]; a -inf logit adds exp = 0 and gets a gradient of exactly 0; +inf
 * is not covered.  A row whose target lies outside [0, N) is never dereferenced with it: row loss 0, gradient row 0, rank N, and it
 * counts in *skipped (a device int32, overwritten); the mean still divides by B.
 * A row is reduced in chunks of ffwm_softmax_xent_chunk() elements, the chunks' sums meet in double in an order fixed by the
 * shapes: two calls agree bit for bit.  workspace: ffwm_softmax_xent_workspace_bytes bytes, 8-byte aligned, contents irrelevant on
 * entry and exit (a negative ffwm_status for sizes the entry point refuses).  N up to 2^24, B up to 65535; beyond: FFWM_ERR_SIZE. */
int ffwm_softmax_xent_chunk(void);
int64_t ffwm_softmax_xent_workspace_bytes(int64_t B, int64_t N, int dtype);
int ffwm_softmax_xent(const void* logits, const int64_t* target, void* out, void* row_loss, int* rank, void* grad_logits,
                      int* skipped, void* workspace, int64_t B, int64_t N, int dtype, void* stream);

/* ---- netG eval forward (models/base_networks.py:274-347): the layers around the dense convolutions once BatchNorm is folded
 * into the conv weights (ffwm_amd/ffwm_eval.py, csrc/netg_eval.hip).  float32, forward only.
 *
 * A DESTINATION VIEW is a [B, C, H, W] view whose samples are contiguous: sample b starts at y + b * y_batch_stride.  A channel
 * slice of the decoder's concatenation buffer is one, so cat(skip * att, dec, up(recon)) (:334-340) is written in place by the
 * three producers and never copied.  Every entry point returns FFWM_ERR_DTYPE for a dtype other than FFWM_F32, FFWM_ERR_ARG for
 * a NULL tensor pointer, a non-positive size or a batch stride smaller than one sample of the view, FFWM_ERR_SIZE for a plane
 * past its index range -- all before any launch.
 *
 * ffwm_shuffle_bias_act_forward: PixelShuffle(2) -> per-channel shift -> LeakyReLU of a decoder block (:261-272) in one pass:
 *   y[b, k, 2 yy + i, 2 xx + j] = lrelu(h[b, 4 k + 2 i + j, yy, xx] + bias[k]),  h [B, 4 K, H, W] contiguous, bias [K] or NULL,
 *   y a destination view [B, K, 2 H, 2 W].
 * ffwm_image_head_forward: y = sigmoid(conv2d(x[B, C, H, W], weight[3, C, 3, 3], stride 1, pad 1) + bias[3]) (rec0 / rec1 / rec2,
 *   :303-305) by a direct kernel staged through LDS, any H and W; y a destination view [B, 3, H, W].  Partial sums meet in a fixed
 *   order: bit-reproducible.
 * ffwm_upsample2x_bilinear_forward: F.interpolate(x[B, C, H, W], scale_factor=2, mode="bilinear") with align_corners=False (:337)
 *   into a destination view [B, C, 2 H, 2 W].
 * ffwm_sigmoid_gate_forward_strided: ffwm_sigmoid_gate_forward (same arithmetic, same order) on [B, C, HW] tensors with y in a
 *   destination view; att (contiguous) may be NULL: not written. */
int ffwm_shuffle_bias_act_forward(const void* h, const void* bias, void* y, int64_t B, int64_t K, int64_t H, int64_t W,
                                  int64_t y_batch_stride, double negative_slope, int dtype, void* stream);
int ffwm_image_head_forward(const void* x, const void* weight, const void* bias, void* y, int64_t B, int64_t C, int64_t H, int64_t W,
                            int64_t y_batch_stride, int dtype, void* stream);
int ffwm_upsample2x_bilinear_forward(const void* x, void* y, int64_t B, int64_t C, int64_t H, int64_t W, int64_t y_batch_stride,
                                     int dtype, void* stream);
int ffwm_sigmoid_gate_forward_strided(const void* a, const void* b, const void* x, void* att, void* y, int64_t B, int64_t C,
                                      int64_t HW, int64_t y_batch_stride, int dtype, void* stream);

/* ---- identity evaluation (csrc/lightcnn_eval.hip): float32 only, FFWM_ERR_DTYPE otherwise ----------------------------------
 * The tail of a LightCNN layer as one pass: h [B, 2C, H, W] is the convolution without its bias, bias [2C] or NULL, residual
 * [B, C, H, W] or NULL, pool 0 / 1 = MaxPool2d(2, 2, ceil_mode=True) (a window that hangs over the edge takes its in-bounds elements):
 *     y = pool(max(h[:, :C] + bias[:C], h[:, C:] + bias[C:]) + residual),   y [B, C, H, W] or [B, C, ceil(H / 2), ceil(W / 2)]
 * contiguous.  Equal to the PyTorch composition bit for bit; NaN propagates as in ATen's maximum and max_pool2d. */
int ffwm_mfm_tail_forward(const void* h, const void* bias, const void* residual, void* y, int64_t B, int64_t C, int64_t H, int64_t W,
                          int pool, int dtype, void* stream);
/* The identity network's input from img [B, Cin, H, W] into out [B, 1, H, W].  crop 0: the channel mean (a left-to-right sum, one
 * division).  crop 1 (H = W = 128 only): mean -> WarpNet(build_grid(B, 98)) -> bilinear resize to 128 x 128 (models/losses.py:85-112)
 * as one 16-tap gather per output pixel. */
int ffwm_identity_input(const void* img, void* out, int64_t B, int64_t Cin, int64_t H, int64_t W, int crop, int dtype, void* stream);
/* The adjoint of ffwm_identity_input: grad_out [B, 1, H, W] -> grad_img [B, Cin, H, W], OVERWRITTEN (every element written exactly
 * once; no zero-fill needed).  crop 0: grad_out / Cin into every channel.  crop 1 (H = W = 128 only): the forward is the separable
 * linear map out = A_y gray A_x^T (A = resize x sample per axis, from the forward's own coordinates), so grad_img[b, c] =
 * A_y^T grad_out[b, 0] A_x / Cin, as a gather over the few outputs that touch each input cell, summed in ascending output order:
 * no atomics, bit-identical from run to run, exactly 0 in rows 0 .. 26 and 127 and columns 0 .. 13 and 114 .. 127 (no tap of the
 * forward reaches them).  Same argument checks as ffwm_identity_input. */
int ffwm_identity_input_backward(const void* grad_out, void* grad_img, int64_t B, int64_t Cin, int64_t H, int64_t W, int crop, int dtype,
                                 void* stream);
/* torch.cosine_similarity (eps 1e-8 on each norm) of probe [B, D] against gallery [G, D] and its k best per probe: values [B, k]
 * float32 descending, indices [B, k] int32; equal similarities: the lower index first; a NaN similarity ranks above everything.
 * 1 <= k <= min(G, 32), D <= 1024, B <= 65535.  Deterministic, no atomics.  workspace: 16-byte aligned, at least
 * ffwm_cosine_topk_workspace_bytes (0 for sizes the entry refuses) bytes; nothing in it needs to be initialised. */
int64_t ffwm_cosine_topk_workspace_bytes(int64_t B, int64_t G, int64_t D, int64_t k);
int ffwm_cosine_topk(const void* probe, const void* gallery, void* values, void* indices, int64_t B, int64_t G, int64_t D, int64_t k,
                     void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- device-resident face dataset (csrc/face_batch.hip): the reference's data/face_dataset.py with --preload ----------------
 * The store stays on the device as bytes; ONE launch assembles a batch from a DEVICE vector of item indices (a captured launch
 * follows the contents of that vector).
 *   images uint8 [N, H, W, 3] (RGB), masks uint8 [N, H, W]; pairs int32 [P, 2]: the rows of S and F of every pair;
 *   pair_lm int32 [P, 3]: the rows of lm_S and lm_F in the landmark tables and the row of the gate table;
 *   lm / lm_flip int32 [K, L, 2]: the landmarks as the reference delivers them (long(), clamped) without and with the flip's
 *   x -> 127 - x, both worked out once on the host in the reference's own arithmetic; gate float32 [KG, L]; index int32 [B].
 * train 1: index i in [0, 2 P), i >= P is the flipped copy (images and masks reversed along W, lm_flip) of pair i - P.  Written:
 *   img_S / img_F float32 [B, 3, H, W], mask_S / mask_F float32 [B, 1, H, W] = byte / 255 (a true division), lm_S / lm_F int64
 *   [B, L, 2], gate_out float32 [B, L, 1], invalid int32 [B].
 * train 0 (a test batch): index in [0, P), nothing is flipped, only img_S, img_F and invalid are written; masks, pair_lm, the tables
 *   and the other outputs are not looked at (NULL allowed).
 * Every output element is written exactly once by a plain store (no zero-fill needed, nothing else is touched).  An index outside its
 * range, or a table row outside its table, is never used as an address: that sample's outputs are zeros and invalid[b] = 1 (else 0).
 * Before any launch: FFWM_ERR_ARG for a NULL pointer that the mode needs or a size <= 0, FFWM_ERR_SIZE for H or W > 8192, B > 65535,
 * L > 2^20, N >= 2^31 or P >= 2^30. */
int ffwm_face_batch(const void* images, const void* masks, const void* pairs, const void* pair_lm, const void* lm, const void* lm_flip,
                    const void* gate, const void* index, void* img_S, void* img_F, void* mask_S, void* mask_F, void* lm_S, void* lm_F,
                    void* gate_out, void* invalid, int64_t N, int64_t H, int64_t W, int64_t P, int64_t K, int64_t KG, int64_t L,
                    int64_t B, int train, void* stream);
/* The same training batch with the S side rotated: the random rotation of the reference's --aug (face_dataset.py:110-130) by a whole
 * angle per sample, STATED as the classic bilinear path of cv2.warpAffine (no OpenCV was at hand to confirm its bytes).  Beside the
 * arguments of ffwm_face_batch:
 *   lm_raw / lm_raw_flip float32 [K, L, 2]: the landmark rows before .long() (plain, and after x -> 127 - x), row for row beside lm;
 *   slot int32 [B] (device): the angle slot of every sample, in [0, A);  A in [1, 64];
 *   xtab int32 [A, 2, W]: adelta[x] = rint(M0 x 1024), bdelta[x] = rint(M3 x 1024);  ytab int32 [A, 2, H]: X0[y] = rint((M1 y + M2)
 *   1024) + 16, Y0[y] = rint((M4 y + M5) 1024) + 16 of warpAffine's inverted matrix M, made on the host once per angle and size;
 *   cs float32 [A, 2]: cos and sin of -angle rounded to float32;  load_size: the centre of the landmark rotation is load_size / 2.
 * Per pixel of img_S / mask_S: X = (X0[y] + adelta[x]) >> 5, Y = (Y0[y] + bdelta[x]) >> 5, S = the four taps at (Y >> 5, X >> 5) of
 *   the (flipped, where index >= P) image under the weights (32 - fx)(32 - fy), fx (32 - fy), (32 - fx) fy, fx fy of fx = X & 31, fy =
 *   Y & 31, a tap outside the image 0; img_S = float(S) / 1024 / 255 (exact up to the true division), mask_S = S > 0 ? 1 : 0.
 * lm_S = the reference's float32 chain on the raw row: x0 = x - h, y0 = y - h (h = load_size / 2), x' = (x0 c - y0 s) + h, y' = (x0 s
 *   + y0 c) + h, every product and sum rounded to float32 on its own, clipped to [0, load_size], truncated, clamped to load_size - 1.
 * img_F, mask_F, lm_F, gate_out and the rule for invalid samples are those of ffwm_face_batch; a slot outside [0, A) is invalid too.
 * One launch, every output element written once by a plain store, nothing else; the source rows a block needs are staged in LDS when
 * they fit 32 KiB + 64 B and read from global memory otherwise.  Tables are only ever indexed inside their bounds and every tap is
 * checked against the rows at hand: wrong table CONTENTS give wrong pixels, never an address outside the store.
 * Before any launch: the checks of ffwm_face_batch, and FFWM_ERR_ARG for train != 1, a NULL pointer among the new ones, load_size <=
 * 0, A < 1 or A > 64; FFWM_ERR_SIZE for load_size > 2^24. */
int ffwm_face_batch_aug(const void* images, const void* masks, const void* pairs, const void* pair_lm, const void* lm,
                        const void* lm_flip, const void* gate, const void* index, const void* lm_raw, const void* lm_raw_flip,
                        const void* slot, const void* xtab, const void* ytab, const void* cs, void* img_S, void* img_F, void* mask_S,
                        void* mask_F, void* lm_S, void* lm_F, void* gate_out, void* invalid, int64_t N, int64_t H, int64_t W, int64_t P,
                        int64_t K, int64_t KG, int64_t L, int64_t B, int64_t A, int64_t load_size, int train, void* stream);
/* Gallery planes: out float32 [G, 1, H, W] = ((r + g) + b) / 3 of byte / 255 of image rows[g] (int32 [G], device) -- the arithmetic
 * of ffwm_identity_input (crop 0) on the float image.  A row outside [0, N) gives a plane of zeros.  Same argument checks. */
int ffwm_face_gallery(const void* images, const void* rows, void* out, int64_t N, int64_t H, int64_t W, int64_t G, void* stream);
/* LightCNN fine-tuning batches (csrc/identity_batch.hip): the reference's lightcnn/dataset.py with --preload in ONE launch.
 *   images uint8 [N, H, W, 3], targets int64 [N], index int32 [B], matrix float64 [B, 6], flip uint8 [B]: all on the device (a
 *   captured launch follows the contents of index, matrix and flip).
 * augment 1 (a training item): image index[b] rotated as PIL's Image.rotate(angle, BICUBIC, expand=False) rotates it under the
 *   inverse-map matrix[b] (xin = m0 (x + .5) + m1 (y + .5) + m2, yin = m3 .. m5; outside the image 0; the a = -1 cubic over 4 x 4
 *   index-clamped taps in float64, clipped and truncated to a byte), mirrored along W where flip[b] != 0, byte / 255 in float32,
 *   channel mean ((r + g) + b) / 3.  augment 0 (a test item): byte / 255 and the mean only; matrix and flip are not looked at (NULL
 *   allowed).
 * crop 1: the slice [28:-2, 15:-15] of that plane resized to out_side x out_side as upsample_bilinear2d (align_corners false) in
 *   float32.  crop 0: out_side is not looked at.
 * Written: img float32 [B, 1, H, W] (crop 0) or [B, 1, out_side, out_side] (crop 1), target int64 [B] = targets[index[b]], invalid
 *   int32 [B]; every element exactly once by a plain store, nothing else.  A sample whose index is outside [0, N) or, with augment,
 *   whose matrix has an entry that is not finite is never used as an address: zeros, target 0, invalid[b] = 1 (else 0).  Any finite
 *   matrix is safe: the inside test is made before a coordinate becomes an integer.
 * Before any launch: FFWM_ERR_ARG for a NULL pointer that the mode needs, a size <= 0, augment or crop outside {0, 1}, crop with
 *   H <= 30 or W <= 30; FFWM_ERR_SIZE for H, W or out_side > 8192, B > 65535, N >= 2^31, or a crop whose band of 8 output rows reads
 *   more than 64 KiB of plane rows. */
int ffwm_identity_batch(const void* images, const void* targets, const void* index, const void* matrix, const void* flip, void* img,
                        void* target, void* invalid, int64_t N, int64_t H, int64_t W, int64_t B, int64_t out_side, int augment,
                        int crop, void* stream);

/* ---- result images (csrc/visuals.hip): the reference's util/util.py tensor2im / tensor2mask / tensor2flow / tensor2att and
 * util/flow_util.py flow2img for whole batches, every visual of a call in one pass.  An item is one visual:
 *   src      float32 [B, C, H, W], contiguous, 4-byte aligned (16-byte aligned with H*W % 4 == 0 takes the float4 path)
 *   out      uint8 [B, H, W, 3], RGB in HWC order, 4-byte aligned; every byte written exactly once by a plain store, nothing else
 *   palette  kind 3 only: uint8 [256, 3] RGB on the device (the library ships no colour map)
 *   kind     0 IMAGE   C == 3: u8(x * 255);  C == 1: u8(((x - 0.5) * 2) * 255) on all three channels
 *            1 MASK    u8(x * 255), C == 1 tiled to three channels; C is 1 or 3
 *            2 FLOW    C == 2: g = clamp((f + 1) * (H / 2), 0, H - 1) in float32 (both axes scale with H; NaN passes), u = g[0] - x,
 *                      v = g[1] - y, rad = sqrtf(u u + v v); per image m = max(rad), NaN if any cell is NaN, maxrad = m > -1 ? m : -1;
 *                      u' = (double)(u / maxrad) + DBL_EPSILON (v' alike; float32 division, float64 from there on); a cell whose u' or
 *                      v' is NaN is black; fk = (atan2(-v', -u') / pi + 1) / 2 * 54 + 1, k0 = floor(fk), k1 = k0 + 1 (56 -> 1),
 *                      f = fk - k0; per channel col = (1 - f) wheel[k0 - 1] / 255 + f wheel[k1 - 1] / 255 over the 55-entry Middlebury
 *                      wheel; rad' = sqrt(u' u' + v' v') <= 1: col = 1 - rad' (1 - col), else col *= 0.75; byte = floor(255 col)
 *            3 PALETTE palette[u8(x[:, 0] * 255)], C >= 1
 *   u8(t): truncate toward zero to int32, keep the low 8 bits; NaN, +-inf and |t| >= 2^31 give 0.
 * Items may differ in size; at most 16 per call.  workspace: one float per image of the FLOW items (ffwm_visuals_workspace_bytes;
 * NULL / 0 without one), written by a first launch (one workgroup per flow image, no atomics) and read by the colouring launch; a
 * call without a flow item is one launch.  float32 only: any other dtype returns FFWM_ERR_DTYPE.
 * Before any launch: FFWM_ERR_ARG for a NULL table, src or out, n outside 1 .. 16, a kind outside 0 .. 3, a C the kind does not
 * take, a non-positive size, a palette item without palette, a misaligned pointer, a workspace that is missing or too small;
 * FFWM_ERR_SIZE for B*H*W >= 2^31.  ffwm_visuals_workspace_bytes returns the same negative status for such a table. */
typedef struct ffwm_visual_item {
    const void* src;
    const void* palette;
    void* out;
    int kind;
    int64_t B, C, H, W;
} ffwm_visual_item;
int64_t ffwm_visuals_workspace_bytes(const ffwm_visual_item* items, int n);
int ffwm_visuals(const ffwm_visual_item* items, int n, void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- built-in per-kernel timing (HIP events on the launch stream) ---------------------------
 * ffwm_prof_enable(1) brackets every kernel launch of this library with a pair of HIP events
 * recorded on the stream the kernel is launched on.  ffwm_prof_collect() waits for the recorded
 * events, folds them into per-kernel totals and returns the number of distinct kernels seen;
 * ffwm_prof_get() reads one row.  ffwm_prof_reset() drops everything. */
int ffwm_prof_enable(int on);
int ffwm_prof_collect(void);
int ffwm_prof_get(int row, char* name, int name_len, int64_t* launches, double* total_ms,
                  double* algorithmic_bytes);
/* total algorithmic flops of row `row` (non-zero for the MFMA kernels: conv3x3_wgrad, correlation_colmax) */
int ffwm_prof_get_flops(int row, double* algorithmic_flops);
/* Sum over the row's launches of max(algorithmic bytes / 8 TB/s, algorithmic flops / 157.3 TFLOP/s), in ms: the time the BINDING
 * roofline of each launch allows.  A scope that serves many shapes (a weight gradient from 128 x 128 planes down to 2 x 2) is
 * MFMA-bound on some launches and weight-streaming on others; total_ms / this = how far the scope is from its own rooflines. */
int ffwm_prof_get_bound(int row, double* roofline_ms);
int ffwm_prof_reset(void);

/* Tuning switches (bench and tests only; the keys are the members of struct Options in ffwm_amd/csrc/common.hpp).  Returns the
 * previous value of the option.  No option gives a negative value a meaning: an unknown key or value < 0 changes nothing and
 * returns FFWM_ERR_ARG, so a negative return is always an error. */
int ffwm_set_option(const char* key, int value);

/* Zero-fill `bytes` bytes (a multiple of 4) at the 4-byte aligned device address `p` with a KERNEL on `stream` -- what the
 * caller-zero-fills contract of the backward entry points (external_function.py:49-50,96,137-138) needs under hipGraph capture, where
 * hipMemsetAsync becomes a memset node: on ROCm 7.0 such nodes were executed with a corrupted fill pattern when several graphs with
 * side-stream branches were replayed back to back (profiles/r05_wgrad_nan_root_cause.txt). */
int ffwm_zero_fill(void* p, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FFWM_HIP_H_ */

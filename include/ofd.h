/* libofd_hip -- C-ABI of the MI355X-native FlowDiffuser hot path (gfx950 only).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  All pointers are
 * DEVICE pointers unless a parameter says "host".  Every call enqueues work on `stream`
 * (a hipStream_t passed as void*, e.g. torch.cuda.current_stream().cuda_stream) and returns
 * 0 on success or a negative ofd_status; ofd_last_error() gives the message of the last
 * failure on the calling thread.  No call synchronises the device.  The caller owns all
 * buffers; the library owns nothing but the handles it returns.
 *
 * Reference interfaces replaced (paths relative to the reference repo,
 * algorithms/diffusion_animation/):
 *   softsplat_new.py:255-269,352-423  cuda_launch("softsplat_out")      -> ofd_splat_fwd
 *   softsplat_new.py:489-565          cuda_launch("softsplat_ingrad")   -> ofd_splat_bwd_in
 *   softsplat_new.py:600-700          cuda_launch("softsplat_flowgrad") -> ofd_splat_bwd_flow
 *   warp.py:121-156   warp_forward_flow (NaN handling + holes)          -> ofd_warp_prep / ofd_warp_holes
 *   warp.py:95-119    warp_backward_flow (2x F.grid_sample + mask)      -> ofd_grid_warp_fwd, ofd_grid_warp_bwd
 *   denoising_diffusion.py:363-417    Unet.forward                      -> ofd_unet_forward
 *   denoising_diffusion.py:666-698    p_mean_variance + p_sample update -> ofd_ddpm_update(_obj)
 *   denoising_diffusion.py:750-767    ddim_sample update                -> ofd_ddim_update(_obj)
 *   (not in the reference)            DPM-Solver++ multistep update     -> ofd_dpmpp_update
 *   (not in the reference)            constrained (inpainting) updates  -> ofd_ddpm_update_known, ofd_ddim_update_known,
 *                                                                          ofd_dpmpp_update_known
 *   (not in the reference)            classifier-free guided updates    -> ofd_ddpm_update_guided, ofd_ddim_update_guided,
 *                                                                          ofd_dpmpp_update_guided
 *   (not in the reference)            condition dropout (CFG training)  -> ofd_cond_drop
 *   (not in the reference)            dynamic thresholding              -> ofd_x0_abs_quantile, ofd_ddpm_update_thresh,
 *                                                                          ofd_ddim_update_thresh, ofd_dpmpp_update_thresh
 *   (not in the reference)            photometric guidance of sampling  -> ofd_photo_pyramid, ofd_photo_guide
 *   (not in the reference)            two-frame interpolation (softmax splatting) -> ofd_interp_prep, ofd_interp_merge
 *   (not in the reference)            joint bilateral upsampling (reduced-size sampling) -> ofd_joint_upsample
 *   (not in the reference)            looping clips from a steady motion field -> ofd_flow_integrate, ofd_loop_render
 *   (not in the reference)            forward-backward check of a flow pair -> ofd_flow_consistency
 *   (not in the reference)            tracks through a clip's flows, layer propagation -> ofd_flow_chain, ofd_flow_chain_to, ofd_layer_composite
 *   (not in the reference)            motion-compensated temporal filter of a clip, along its tracks -> ofd_temporal_filter
 *   (not in the reference)            flow-guided completion of a masked region of a clip, along its tracks -> ofd_clip_fill
 *   (not in the reference)            membrane of a masked region (multigrid Laplace solve), seamless fills -> ofd_membrane_solve
 *   (not in the reference)            guided weighted median of a flow  -> ofd_flow_median
 *   (not in the reference)            global motion of a flow: robust fit, split, render -> ofd_motion_fit, ofd_motion_field, ofd_homography_warp
 *   (not in the reference)            motion layers: K motions of a flow, labels, label vote -> ofd_motion_layers, ofd_motion_assign, ofd_label_vote
 *   (not in the reference)            background plate of a clip: temporal median mosaic, projection -> ofd_plate_reduce, ofd_plate_project
 *   denoising_diffusion.py:806-812    q_sample                          -> ofd_q_sample
 *   denoising_diffusion.py:844-879,985-993  p_losses noise / target     -> ofd_diffusion_prep
 *   denoising_diffusion.py:73-77      (un)normalize                     -> ofd_range_map
 *   warp.py:260-271 + denoising_diffusion.py:908,973  nan_mse + nanmean -> ofd_nan_mse_sum
 *   diffusion_animation.py:159-175    FlowCompleter._sparse_from_dense  -> ofd_sparse_flow_sample
 *   diffusion_animation.py:10-11,177-183  weighted_mse_loss (flow norm) -> ofd_completer_loss(_grad)
 */
#ifndef OFD_H
#define OFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OFD_OK = 0,
    OFD_ERR_ARG = -1,       /* bad shape / null pointer / unsupported configuration */
    OFD_ERR_HIP = -2,       /* a HIP runtime call failed */
    OFD_ERR_WORKSPACE = -3, /* workspace too small */
    OFD_ERR_STATE = -4      /* handle used out of order (e.g. forward before weights) */
} ofd_status;

int ofd_version(void);               /* (major << 16) | minor */
const char* ofd_last_error(void);    /* thread-local, never NULL */

/* ---------------------------------------------------------------- forward splat (SS) ------
 * Tensors are contiguous NCHW fp32.  in: (B,C,H,W), flow: (B,2,H,W) with channel 0 = x
 * displacement, out: (B,C,H/scale,W/scale).  out is fully overwritten (no zero-fill needed).
 * radius: half-width in source pixels of the window an output tile scans (>= the expected
 * max |flow| + 1; samples that land farther are still handled, through a slower list pass).
 * workspace: ofd_splat_workspace_bytes(B,H,W) bytes. */
size_t ofd_splat_workspace_bytes(int B, int H, int W);
int ofd_splat_fwd(const float* in, const float* flow, float* out, int B, int C, int H, int W,
                  int scale, int offset_x, int offset_y, int radius,
                  void* workspace, size_t workspace_bytes, void* stream);
/* optional debug output of softsplat_out's integer corner (x0,y0) per source pixel, int32
 * (B,H,W,2), -2^30 where the sample is skipped (non-finite).  Used by the index parity tests. */
int ofd_splat_corners(const float* flow, int32_t* corners, int B, int H, int W,
                      int scale, int offset_x, int offset_y, void* stream);
int ofd_splat_bwd_in(const float* flow, const float* outgrad, float* ingrad, int B, int C, int H, int W,
                     int scale, int offset_x, int offset_y, void* stream);
int ofd_splat_bwd_flow(const float* in, const float* flow, const float* outgrad, float* flowgrad,
                       int B, int C, int H, int W, int scale, int offset_x, int offset_y, void* stream);

/* All L*L offsets of a scale-L splat at once (the photometric pyramid of flow_learner.py:159-206 evaluates every offset of 10
 * levels on the same image and flow).  T: (B, C, L*(H/L), L*(W/L)) with
 *     T[n, c, L*cy + b, L*cx + a] = ofd_splat_fwd(..., scale = L, offset_x = a, offset_y = b)[n, c, cy, cx].
 * One scale-1 splat of the pixels whose targets avoid the reference's border branches for every offset + one separable
 * tent filter of half-width L + a scatter of the remaining pixels with the reference's own remap; L in 1..16.
 * bwd: ingrad (B,C,H,W) and / or flowgrad (B,2,H,W) (either may be NULL) = the sums over (a, b) of ofd_splat_bwd_in /
 * ofd_splat_bwd_flow with the matching slices of dT.  Workspace: ofd_splat_pyramid_workspace_bytes. */
size_t ofd_splat_pyramid_workspace_bytes(int B, int C, int H, int W);
int ofd_splat_pyramid_fwd(const float* in, const float* flow, float* T, int B, int C, int H, int W, int L, int radius,
                          void* workspace, size_t workspace_bytes, void* stream);
int ofd_splat_pyramid_bwd(const float* in, const float* flow, const float* dT, float* ingrad, float* flowgrad,
                          int B, int C, int H, int W, int L, void* workspace, size_t workspace_bytes, void* stream);

/* Photometric loss of one pyramid level on two ofd_splat_pyramid_fwd results in "soft" form (flow_learner.py:176-190):
 * Tin, Ttg: (B, C+1, Ht, Wt), last channel = splatted weight.  filled = Tin_c / (w + 1e-7) where w > 0, NaN elsewhere
 * (fill_holes_nan, WP:273-276); tgt = Ttg_c / (w_t + 1e-7); Charbonnier sqrt(d^2 + 1e-6) (WP:278-287) over the pairs without NaN,
 * per offset: sums / counts [L][L] (row = offset_y, col = offset_x), fp64.  The level loss is mean(sums / counts).
 * bwd: dTin = d(level loss)/dTin x gscale[0] (device scalar). */
int ofd_pyramid_charbonnier_fwd(const float* Tin, const float* Ttg, double* sums, double* counts, int B, int C, int Ht, int Wt,
                                int L, void* stream);
int ofd_pyramid_charbonnier_bwd(const float* Tin, const float* Ttg, const double* counts, const float* gscale, float* dTin,
                                int B, int C, int Ht, int Wt, int L, void* stream);

/* warp_forward_flow pieces (WP:121-156).
 * prep : first (B,C,H,W) -> ten_in (B,C+1,H,W) = cat(nan_to_zero(first) * w, w), w = 0 where any
 *        channel of the pixel is NaN else 1.  square != 0 squares the values (get_variance).
 * holes: splat result (B,C+1,Ho,Wo) -> img (B,C,Ho,Wo); mode 0 = raw sums ("linear_unn"),
 *        mode 1 = divide by (weight + 1e-7) ("linear"); set_nans != 0 puts NaN where weight <= 0. */
int ofd_warp_prep(const float* first, float* ten_in, int B, int C, int H, int W, int square, void* stream);
int ofd_warp_holes(const float* splat, float* img, int B, int C, int Ho, int Wo, int mode, int set_nans, void* stream);

/* Push-pull hole filling (Gortler et al., "The Lumigraph", 1996, section 3.4).  An addition: the reference's fill_holes_nan
 * (WP:273-276) only writes NaN where nothing was splatted, nothing fills the holes.  All arithmetic fp32.
 * x: (B,C,H,W), weight: (B,1,H,W) or NULL (= 1), out: (B,C,H,W), never NaN.  premultiplied == 0: x is a colour image and weight its
 * confidence; != 0: x is the splat accumulator sum(colour * splat weight) and weight the accumulated splat weight, i.e. channels :C
 * and C of ofd_splat_fwd's result.  Layout: x and weight are two contiguous tensors, EXCEPT when weight == x + C*H*W: then they
 * are read in place as the planes of one contiguous (B,C+1,H,W) splat result (sample stride (C+1)*H*W for both; no copy is needed).
 *   level 0  bad = any channel of x non-finite, or weight NaN or <= 0; w0 = bad ? 0 : min(gain * weight, 1);
 *            c0 = (premultiplied ? x / weight : x) * w0, 0 where bad.
 *   pull     H' = ceil(H / 2): S_w, S_c = 2x2 block sums (children outside the level count 0); w' = min(S_w, 1), c' = S_c / max(S_w, 1);
 *            up to the 1x1 level, f = w > 0 ? c / w : 0 there (a sample without a valid pixel comes back as zeros).
 *   push     f_l = c_l + (1 - w_l) * up2(f_{l+1}), up2 = x2 bilinear, half-pixel centres (taps 9/16, 3/16, 3/16, 1/16), edge-clamped.
 * Three launches for any size, no atomics, fixed summation order: the same input gives the same bits.  gain: finite, >= 1.
 * workspace: ofd_pushpull_workspace(B,C,H,W) bytes (0 for a bad shape), 16-byte aligned; a smaller one is an error. */
size_t ofd_pushpull_workspace(int B, int C, int H, int W);
int ofd_pushpull_fill(const float* x, const float* weight, float* out, void* workspace, size_t workspace_bytes,
                      int B, int C, int H, int W, int premultiplied, float gain, void* stream);

/* Frame interpolation by softmax splatting (Niklaus & Liu, "Softmax Splatting for Video Frame Interpolation", CVPR 2020), extended by a
 * forward-backward flow term.  An addition: the reference's softsplat(strMode="soft") leaves the importance metric to the caller and
 * merges nothing.  Both frames are splatted to every time t_k with ofd_splat_fwd and blended; ofd_pushpull_fill closes what both leave
 * open.  These two calls are the passes before and after the splat.  All arithmetic fp32.
 * frame1, frame2: (B,C,H,W); flow12, flow21: (B,2,H,W) in pixels, channel 0 = x, frame1(p) ~ frame2(p + flow12(p)) -- the convention of
 * ofd_splat_fwd and ofd_photo_guide, not the flipped one of ofd_grid_warp_fwd.  times: n floats on the DEVICE, each in [0, 1] (the caller
 * checks the range: no call reads device memory on the host).
 *   metric   for direction a -> b ((1, 2) and (2, 1)) at pixel p = (x, y), q = p + flow_ab(p) (one fp32 addition per axis):
 *            inside = 0 <= q.x <= W-1 and 0 <= q.y <= H-1 (false for a non-finite q).  Bilinear reads at q: x0 = floor(q.x),
 *            x1 = min(x0 + 1, W-1), tx = q.x - x0, likewise in y; value = (1-ty) * ((1-tx) * g00 + tx * g01) + ty * ((1-tx) * g10 + tx * g11).
 *            d = (sum over c, ascending, of |a_c(p) - b_c(q)|) / C;  r = flow_ab(p) + flow_ba(q);  |r| = sqrt(r.x^2 + r.y^2);
 *            z = -alpha * d - beta * |r| where inside, z = -alpha * oob elsewhere;  Z = clamp(z, -zmax, 0), and Z = -zmax where z is NaN
 *            (a NaN of b or flow_ba under q: the worst match).  Z <= 0: exp(Z) cannot overflow.
 *            v = 1 if every channel of a(p) and both components of flow_ab(p) are finite, else 0.
 *   sources  for time t = times[k]: s = 1 - t for frame 1, t for frame 2;  m = s * exp(Z) where v = 1, else 0;
 *            ten_in[dir, b, k] = (a_c * m for the C channels [0 where v = 0], m, v): C + 2 planes;
 *            flows[dir, b, k] = t * flow12 (dir 0), (1 - t) * flow21 (dir 1): one fp32 multiply (1 - t is one fp32 subtraction).
 *            ten_in: (2,B,n,C+2,H,W), flows: (2,B,n,2,H,W): the input and flow of ONE ofd_splat_fwd call on 2*B*n samples of C+2 channels,
 *            whose result is `acc` below.  (A sample whose flow is non-finite at p is skipped by the splat and has v = 0 anyway.)
 *   merge    acc: (2,Bn,C+2,H,W), Bn = B*n.  S_c, M, K = acc[0] + acc[1] of the colour, m and v planes (one fp32 addition each).
 *            colour (Bn,C,H,W) = S_c / M where M > 0 (C divisions per pixel, no reciprocal: M may be tiny), NaN elsewhere (M = 0 or NaN);
 *            weight (Bn,1,H,W) = K where M > 0, else 0: the UNSCALED coverage, so that a pixel one frame covers fully has confidence 1 in
 *            ofd_pushpull_fill(colour, weight, premultiplied = 0) and keeps its colour however small exp(Z) is.
 * One launch each, both directions in the prep's; no atomics, no host sync, the same input gives the same bits.  Loads and stores are
 * 16 bytes wide where W % 4 == 0 (merge: H*W % 4 == 0) and the pointers are 16-byte aligned.  1 <= n <= 64, 1 <= C <= 8;
 * alpha, beta, oob, zmax finite and >= 0.  Outputs must not alias inputs. */
int ofd_interp_prep(const float* frame1, const float* frame2, const float* flow12, const float* flow21, const float* times, int n,
                    float alpha, float beta, float oob, float zmax, float* ten_in, float* flows, int B, int C, int H, int W, void* stream);
int ofd_interp_merge(const float* acc, float* colour, float* weight, int Bn, int C, int H, int W, void* stream);

/* Joint bilateral upsampling (Kopf, Cohen, Lischinski & Uyttendaele, "Joint Bilateral Upsampling", SIGGRAPH 2007).  An addition: the
 * reference samples at the frame's own size only.  A field computed on a frame box-reduced by s is carried back to the frame's size;
 * each output pixel takes its value from the low-resolution neighbours whose guide colour matches its own, so an edge of the field
 * snaps to the edge of the full-resolution guide instead of being smeared across it.  All arithmetic fp32.
 * lo: (B,C,h,w), guide_lo: (B,Cg,h,w) (the guide at low resolution, e.g. its s x s box average), guide: (B,Cg,H,W), out: (B,C,H,W) with
 * H = h*s, W = w*s.  Per sample and output pixel (x, y):
 *   window   nx = 2x + 1 - s and i0 = floor(nx / (2s)) in integers (the low-resolution cell whose centre lies at or left of the pixel's
 *            centre; -1 at the left border), fx = (nx - 2s*i0) / (2s) in [0, 1): one fp32 division of two exact integers.  The taps
 *            are the columns i = i0 - radius + 1 ... i0 + radius; j0, fy and the rows j likewise from y.  Rows run j ascending, and
 *            within a row i ascending.
 *   skipped  a tap outside [0, w-1] x [0, h-1]; a tap where any of the C values of lo is non-finite.
 *   score    dx = (i - i0) - fx, dy = (j - j0) - fy;  d2 = (sum over c, ascending, of (guide_c(x,y) - guide_lo_c(i,j))^2) / Cg;
 *            z = -(dx*dx + dy*dy) / (2 sigma_s^2) - d2 / (2 sigma_r^2), the denominators 2 * (sigma * sigma) in fp32.  sigma_r = +inf
 *            switches the guide off (d2 / inf = 0).  A tap whose z is NaN (a NaN of either guide, inf / inf) is skipped.  The second
 *            term is evaluated as (the sum over c) * k with k = 1 / (Cg * 2 sigma_r^2) rounded to fp32 once (0 for sigma_r = +inf): two
 *            roundings, as the two divisions have.
 *   output   m = the largest z over the kept taps;  out_c = gain * ((sum of exp(z - m) * lo_c) / (sum of exp(z - m))), one division per
 *            channel, then one multiply.  NaN in all C channels when no tap is kept, or when every kept z is -inf.  The maximum is
 *            formed online: a tap with a larger z rescales both running sums by exp(m_old - z) first.  The quotient is evaluated as
 *            r_c + (sum of exp(z - m) * (lo_c - r_c)) / (sum of exp(z - m)) with r the lo of the pixel's own cell (max(i0, 0),
 *            max(j0, 0)), 0 where that tap is skipped as non-finite: the same number, with a rounding error that scales with the
 *            spread of the taps instead of their size (a constant lo comes back exactly).  A tap whose z is -inf has weight 0
 *            under any maximum and is left out of the sums like a skipped one; the output is the same.
 * gain turns the units of lo into those of out: s for a flow in low-resolution pixels that is wanted in full-resolution pixels.
 * One launch; no atomics, no host sync, the same input gives the same bits.  A workgroup stages the low-resolution window of its 64 x 16
 * output tile in LDS and reads the taps from there, the first term of z from a table of its (s * 2 radius)^2 possible values; guide loads and out stores are 16 bytes wide where W % 4 == 0 and guide and out
 * are 16-byte aligned, scalar otherwise.  1 <= C <= 8, 1 <= Cg <= 4, 2 <= s <= 8, 1 <= radius <= 3; sigma_s finite and > 0; sigma_r > 0,
 * +inf allowed; gain finite; H, W < 2^30 and B*(C+Cg)*H*W < 2^40.  Outputs must not alias inputs.  Argument errors return OFD_ERR_ARG and
 * set ofd_last_error before any GPU work.  Compulsory traffic: 4 * B * (H*W*(Cg + C) + h*w*(Cg + C)) bytes. */
int ofd_joint_upsample(const float* lo, const float* guide_lo, const float* guide, float* out, int B, int C, int Cg, int h, int w, int s,
                       int radius, float sigma_s, float sigma_r, float gain, void* stream);

/* Looping clips from a still and a steady motion field (Chuang et al., "Animating Pictures with Stochastic Motion Textures", SIGGRAPH
 * 2005; Holynski et al., "Animating Pictures with Eulerian Motion Fields", CVPR 2021).  An addition: the reference stops at one raw splat
 * of the still by its flow.  For a field that does not change with time the colour of pixel p in frame k is the still read at the
 * point reached by tracing p BACK through the field for k frames: a gather, no holes, no atomics, no fill.  Cross-fading it with the
 * still traced FORWARD for N - k frames makes frame N equal frame 0: the clip repeats without a jump.  All arithmetic fp32, in the
 * order written here.
 * motion: (B,2,H,W) in pixels per frame, channel 0 = x; the content at p moves to p + motion(p) -- the convention of ofd_splat_fwd and
 * ofd_interp_prep.  A non-finite component of motion is read as 0 ("does not move") wherever it is read.
 *   sample   sample(F, qx, qy) is a bilinear read with edge clamp: sx = min(max(qx, 0), W-1), x0 = floor(sx), x1 = min(x0 + 1, W-1),
 *            tx = sx - x0, likewise in y; value = (1-ty) * ((1-tx) * g00 + tx * g01) + ty * ((1-tx) * g10 + tx * g11).  (A NaN
 *            coordinate -- inf - inf after a displacement overflowed -- is read at 0.)  A point traced past the frame's border reads
 *            the border: its colour is stretched, not lost.
 *   trace    a trace with frame step dt keeps a displacement D per pixel p = (x, y), D = 0 at the start.  One frame is `substeps`
 *            sub-steps of h = dt / substeps (one fp32 division); hh = 0.5f * h.  A sub-step reads at q = ((float)x + D.x, (float)y + D.y):
 *            order 1 (Euler)     v = sample(motion, q);  D = D + h * v;
 *            order 2 (midpoint)  v = sample(motion, q);  Dm = D + hh * v;  vm = sample(motion, p + Dm);  D = D + h * vm.
 *            D_j is D after j frames.
 * ofd_flow_integrate: disp (B, steps+1, 2, H, W), disp[:, j] = D_j, disp[:, 0] = 0.  dt: any finite float, negative traces back; it
 * carries the caller's speed, so the field is never rescaled in a pass of its own.  0 <= steps <= 4096.
 * ofd_loop_render: img (B,C,H,W), finite; video (B, nk, C, H, W): the frames k = k0 .. k0 + nk - 1 of the N-frame loop.  For frame k:
 *            t = (float)k / (float)N;  a = sample(img, p + Db_k), Db the trace with dt = -speed;  b = sample(img, p + Df_{N-k}), Df the
 *            trace with dt = +speed;  out = (1 - t) * a + t * b.  Frame 0 is img (1 * a + 0 * b).  The call keeps no state: every call
 *            traces from D = 0, so the frames of a loop split over several calls have the bits of one call.
 *            workspace: ofd_loop_workspace(B, H, W, nk) bytes (0 for a bad shape), the forward displacements of the call's frames,
 *            8 bytes per pixel and frame; a smaller one is an error (OFD_ERR_WORKSPACE).
 *            1 <= C <= 8, 1 <= N <= 4096, 0 <= k0, 1 <= nk, k0 + nk <= N; speed finite.
 * Both: 1 <= substeps <= 16, order 1 or 2, H, W <= 32768.  One launch (integrate) or two (render: the forward trace into the workspace,
 * then back-trace, gathers and blend); no atomics, no host sync, the same input gives the same bits.  A workgroup owns a 64 x 16 tile, a
 * thread one column of four neighbouring rows: every load and store of a wave covers 64 neighbouring pixels of a row, and no pointer
 * needs more than a float's alignment.  Outputs must not alias inputs.  Argument errors return OFD_ERR_ARG and set ofd_last_error
 * before any GPU work.  B * ceil(H / 16) * ceil(W / 64) < 2^30.  Compulsory traffic of ofd_loop_render: 4 * B * (nk*C*H*W + (C+2)*H*W)
 * bytes. */
int ofd_flow_integrate(const float* motion, float* disp, int B, int H, int W, int steps, int substeps, int order, float dt, void* stream);
size_t ofd_loop_workspace(int B, int H, int W, int nk);
int ofd_loop_render(const float* img, const float* motion, float* video, int B, int C, int H, int W, int N, int k0, int nk, int substeps,
                    int order, float speed, void* workspace, size_t workspace_bytes, void* stream);

/* Forward-backward consistency check of a flow pair (Sundaram, Brox & Keutzer, "Dense Point Trajectories by GPU-accelerated Large
 * Displacement Optical Flow", ECCV 2010; the bound of Meister, Hur & Roth, "UnFlow", AAAI 2018).  An addition: nothing in the reference
 * holds the two directions of a flow against each other.  Following a pixel by flow_ab and coming back by flow_ba should end where it
 * started; where it does not, the pixel is occluded in the other frame or one of the flows is wrong.  All arithmetic fp32, in the order
 * written here.
 * flow12, flow21: (B,2,H,W) in pixels, channel 0 = x, frame1(p) ~ frame2(p + flow12(p)): the convention of ofd_splat_fwd and
 * ofd_interp_prep.  For direction a -> b ((1, 2), then (2, 1)) at pixel p = (x, y), with f = flow_ab(p), the first rule that applies:
 *   5 invalid       a component of f is non-finite.
 *   3 leaves        q = p + f (one fp32 addition per axis) is not inside: inside = 0 <= q.x <= W-1 and 0 <= q.y <= H-1, the test of
 *                   ofd_interp_prep (false for a non-finite q).
 *   4 unmatched     g = the bilinear read of flow_ba at q, by ofd_interp_prep's formula (x0 = floor(q.x), x1 = min(x0 + 1, W-1),
 *                   tx = q.x - x0, likewise in y; value = (1-ty) * ((1-tx) * g00 + tx * g01) + ty * ((1-tx) * g10 + tx * g11)), has a
 *                   non-finite component (a non-finite corner makes it so even under weight 0).
 *   2 inconsistent  r = f + g;  e2 = r.x*r.x + r.y*r.y;  m = (f.x*f.x + f.y*f.y) + (g.x*g.x + g.y*g.y);  bound = a1*m + a2;
 *                   `e2 <= bound` is false.  (A finite g so large that its square overflows gives e2 = m = inf: inf <= inf holds for
 *                   a1 > 0, and bound is NaN for a1 = 0.)
 *   1 released      consistent, but dilate > 0 and some pixel of the frame within Chebyshev distance dilate has a state in {2,3,4,5}.
 *   0 held          every other consistent pixel.
 * known (2,B,2,H,W): flow_ab(p) bit for bit in state 0, NaN in both components otherwise: the `known` of the constrained reverse steps
 * once scaled, i.e. what the samplers hold fixed.  err (2,B,1,H,W): sqrtf(e2) in states 0, 1, 2, NaN otherwise.  state (2,B,1,H,W):
 * uint8.  counts (2,B,6), int32: the number of pixels per state; the call zeroes it with a memset on `stream` and fills it with integer
 * atomics, one instruction per wave and tile.  Index 0 of the leading dimension is direction 1 -> 2.
 * One launch for both directions and all samples; no float atomics, no host sync, the same input gives the same bits.  A workgroup owns
 * a 64 x 16 tile of one direction and sample, a thread 4 neighbouring pixels of a row.  For dilate > 0 it also classifies the ring of
 * dilate pixels around its tile, keeps a byte per position in LDS and takes the (2 dilate + 1)^2 maximum there: no plane in between
 * goes through memory.  dilate == 0 has no ring, LDS or barrier.  Loads and stores are 16 bytes wide (state: 4) where W % 4 == 0 and
 * flow12, flow21, known, err are 16-byte and state 4-byte aligned, one element wide otherwise, with the same bits.  a1, a2 finite and
 * >= 0; 0 <= dilate <= 4; H, W <= 32768; 2 * B * ceil(H / 16) * ceil(W / 64) < 2^30.  Outputs must not alias inputs.  Argument errors
 * return OFD_ERR_ARG and set ofd_last_error before any GPU work.  Compulsory traffic per direction and pixel: 8 B read, 8 + 4 + 1 B
 * written: 42 * B * H * W bytes in all.  The pass is bound by the latency of its gathers (8 corner loads per pixel), not by that. */
int ofd_flow_consistency(const float* flow12, const float* flow21, float a1, float a2, int dilate, float* known, float* err,
                         uint8_t* state, int32_t* counts, int B, int H, int W, void* stream);

/* Guided weighted median of a flow (Sun, Roth & Black, "Secrets of optical flow estimation and their principles", CVPR 2010, in its
 * weighted, image-guided form).  An addition: nothing in the reference cleans a flow.  Every vector is replaced, plane by plane, by the
 * lower weighted median of its (2 radius + 1)^2 window; a neighbour counts by how near it is and by how much its guide colour
 * resembles the centre's, so that isolated wild vectors are voted away while a motion boundary stays on the guide's edge.  Scores are
 * fp32 in the order written here; from the weights on everything is integer arithmetic.
 * flow, out: (B,C,H,W), 1 <= C <= 4; guide: (B,Cg,H,W), 0 <= Cg <= 4, NULL exactly when Cg == 0; conf: (B,1,H,W) or NULL.  For the
 * output pixel p = (x, y) and tap j = (dy + radius) * (2 radius + 1) + (dx + radius), dy outer, dx inner, both ascending from -radius,
 * let q = p + (dx, dy):
 *   confidence  cf = conf(q) clamped to [0, 1], a NaN counting as 0; 1 when conf is NULL.
 *   score       d2 = sum over c, ascending, of (guide_c(p) - guide_c(q))^2;  z = -(dx*dx + dy*dy) / (2 sigma_s^2) - d2 * k_r with
 *               k_r = 1 / (Cg * 2 sigma_r^2): the denominators 2 * (sigma * sigma) in fp32, k_r rounded to fp32 once, the formulas and
 *               operation order of ofd_joint_upsample.  +inf is allowed for either sigma and switches that term off: the first
 *               term is then -0 and k_r is 0.  With Cg == 0 there is no second term: z is the first.  With both terms off every tap
 *               has z = -0.
 *   valid       q is inside the image, all C values of flow at q are finite, and z is not NaN (a NaN of the guide at p or q,
 *               inf * 0).
 *   weight      w_j = (uint32) floorf(expf(z) * cf * 65536 + 0.5), the products from left to right; 0 for a tap that is not valid.
 *               T = the sum of the w_j, at most 49 * 65536.  Integer sums do not depend on their order (the idea of csrc/det.h,
 *               applied to a rank).
 *   result      for each plane c by itself: order the taps by (flow_c(q) ascending, j ascending) under the float <, so that -0.0 and
 *               +0.0 tie and j decides; below_k = the sum of w over the taps before k.  out_c(p) = the BITS of flow_c at the one
 *               tap with w_k > 0 and 2 below_k < T <= 2 (below_k + w_k): the lower weighted median, always one of the window's own
 *               values.  T == 0: the quiet NaN 0x7fc00000 in every plane.
 *   fill        0: a pixel whose own flow is non-finite in some plane is that NaN in every plane, so that a NaN mask such as a
 *               `known` plane passes through.  1: such a pixel gets the weighted median of its valid neighbours (its own tap is
 *               not valid): holes up to radius wide close.
 * One launch; no atomics, no host sync, no branch on data, no float becomes an index; the same input gives the same bits.  A workgroup
 * stages the (64 + 2 radius) x (16 + 2 radius) window of its 64 x 16 tile in LDS, C + Cg + 1 planes, the last being cf with 0 for
 * every position that cannot vote; a thread owns 4 neighbouring pixels of a row, keeps a pixel's weights in registers and finds each
 * plane's median by counting, without a sort.  out stores are 16 bytes wide where W % 4 == 0 and out is 16-byte aligned, one float
 * wide otherwise, with the same bits.  1 <= radius <= 3; sigma_s, sigma_r > 0; fill 0 or 1; H, W <= 32768;
 * B * ceil(H / 16) * ceil(W / 64) < 2^30; B*(C+Cg+1)*H*W < 2^40.  out must not overlap flow, guide or conf: the filter is not in place.
 * Argument errors return OFD_ERR_ARG and set ofd_last_error before any GPU work.  Compulsory traffic: 4 * B * H * W * (2 C + Cg + 1)
 * bytes (+1: conf, where given).  The pass is bound by its vector ALU work -- about 5 operations per pair of taps and plane, 300
 * pairs at radius 2 -- not by that. */
int ofd_flow_median(const float* flow, const float* guide, const float* conf, float* out, int B, int C, int Cg, int H, int W, int radius,
                    float sigma_s, float sigma_r, int fill, void* stream);

/* Flow chaining: dense tracks through a clip, and a painted layer carried along them (the subject of Sundaram, Brox & Keutzer, ECCV
 * 2010, cited above, with UnFlow's bound).  An addition: nothing in the reference looks at more than two frames.  Every pixel of one
 * frame is followed through the consecutive flows of the clip by COMPOSING them -- each flow is read where the track has got to, not
 * at the pixel it started from -- and a track ends where the round trip of a step fails (occlusion), where it leaves the frame, or
 * where a flow is not finite.  This is not ofd_flow_integrate, which walks ONE steady field, clamps at the border and reads NaN as 0.
 * All arithmetic fp32, in the order written here.
 * fwd, bwd: (B,T,2,H,W) in pixels, channel 0 = x.  fwd[:, j] carries frame j to frame j + 1: frame_j(p) ~ frame_{j+1}(p + fwd_j(p)),
 * the convention of ofd_flow_consistency's flow12; bwd[:, j] carries frame j + 1 to frame j.  A clip of T + 1 frames has T of each.
 * One step of a track from frame a to a neighbouring frame uses S, the field that carries a to the neighbour (fwd[:, a] ahead,
 * bwd[:, a - 1] back), and, with the check on, K, the field that carries the neighbour back to a (bwd[:, a] ahead, fwd[:, a - 1] back).
 * A track of the pixel p = (x, y) keeps a displacement D, 0 at the start, and a state, 0 at the start.  A step of a living track:
 *   q = ((float)x + D.x, (float)y + D.y);  v = the bilinear read of S at q by ofd_flow_consistency's formula (x0 = floor(q.x),
 *   x1 = min(x0 + 1, W-1), tx = q.x - x0, likewise in y; value = (1-ty) * ((1-tx) * g00 + tx * g01) + ty * ((1-tx) * g10 + tx * g11); a
 *   non-finite corner makes v non-finite even under weight 0).  q is inside: it is the q' that the step before accepted, or p.
 *   5 invalid       a component of v is non-finite.
 *   D' = D + v;  q' = ((float)x + D'.x, (float)y + D'.y).
 *   3 leaves        q' is not inside: inside = 0 <= q'.x <= W-1 and 0 <= q'.y <= H-1 (false for a non-finite q').
 *   with the check on: g = the bilinear read of K at q'.
 *   4 unmatched     g has a non-finite component.
 *   2 inconsistent  r = v + g;  e2 = r.x*r.x + r.y*r.y;  m = (v.x*v.x + v.y*v.y) + (g.x*g.x + g.y*g.y);  bound = a1*m + a2, exactly as
 *                   in ofd_flow_consistency; `e2 <= bound` is false.  (As there: a finite g so large that its square overflows, such
 *                   as 1e30, gives e2 = m = inf; inf <= inf holds for a1 > 0, so the track lives on, and bound is NaN for a1 = 0, so
 *                   it dies here.  Under weight 0 such a corner is 0 * 1e30 = 0.)
 *   0 tracked       otherwise, and D = D'.
 * The first rule that applies ends the track: it is dead, keeps that state, and its D is the quiet NaN at this and every later frame.
 * The numbers are those of ofd_flow_consistency's states; 1 is not used.
 * ofd_flow_chain: tracks every pixel of frame `start` to frame `stop`, n = |stop - start| steps, ahead (stop >= start: steps by fwd,
 *   checks by bwd) or back (steps by bwd, checks by fwd).  disp (B, n+1, 2, H, W), state (B, n+1, 1, H, W) uint8: slot i holds the
 *   track on arrival at the i-th frame of the walk, slot 0 is D = 0 with state 0.  life (B, 1, H, W) int32: the number of steps
 *   completed alive, 0..n.  all_steps = 0 stores only the last slot: disp (B, 1, 2, H, W), state (B, 1, 1, H, W).  n = 0 is allowed.
 *   The stepping array must be non-null (fwd for stop >= start), the checking array may be null only with use_check = 0.
 * ofd_flow_chain_to: the lookup form.  For every frame t in [t0, t0 + nt) it gives, for each pixel of frame t, its displacement into
 *   frame `anchor` and the final state of that walk of |t - anchor| steps towards the anchor: disp (B, nt, 2, H, W), state
 *   (B, nt, 1, H, W), slot t - t0 with the bits of the last slot of ofd_flow_chain(start = t, stop = anchor).  One launch; all threads
 *   of a workgroup share t.  A frame's result does not depend on how the frames are split over calls.  0 <= t0, 1 <= nt,
 *   t0 + nt <= T + 1; fwd and bwd both non-null.
 * ofd_layer_composite: frames, out (B, n, C, H, W); layer (B, C+1, H, W), premultiplied colour with alpha last; disp (B, n, 2, H, W),
 *   e.g. ofd_flow_chain_to's; 1 <= C <= 8, 1 <= n <= 4097.  With d = disp(p) and q = ((float)x + d.x, (float)y + d.y): where d is finite
 *   and q is inside, out_c = frame_c * (1 - A) + L_c (one subtraction, one product, one sum), A and L_c the bilinear reads of the
 *   layer's planes at q, one cell formed for all C + 1 planes; elsewhere out = frame, bit for bit.  A gather: no holes.
 * All three: one launch; no atomics, no LDS, no host sync; a thread writes only its own pixels; the same input gives the same bits.  A
 * workgroup owns a 64 x 16 tile of one walk (or frame) and sample, a thread one column of four neighbouring rows, so that every load
 * and store of a wave covers 64 neighbouring pixels of a row and no pointer needs more than its element's alignment; the step loop
 * runs in registers.  A float becomes a gather index only after the inside test, which a non-finite or huge value fails; a dead
 * track, and a pixel the composite leaves alone, read at offset 0 of the plane and drop what they read: whatever the fields hold,
 * every read is inside its plane.  H, W <= 32768; 1 <= T <= 4096; 0 <= start, stop, anchor <= T; a1, a2 finite and >= 0; use_check
 * and all_steps 0 or 1; the number of tiles (B, nt * B, B * n times ceil(H / 16) * ceil(W / 64)) < 2^30; every array < 2^40 elements.
 * Outputs must not alias inputs: a thread gathers other pixels' inputs, so an output that shares a byte with an input array is a race,
 * and is rejected.  Argument errors return OFD_ERR_ARG and set ofd_last_error before any GPU work.  Per step and pixel
 * a walk makes 8 corner loads, 16 with the check, each step's behind the one before: it is taken to be bound by the latency of these gathers,
 * like ofd_flow_integrate, whose time it matches, not by its compulsory traffic (ofd_flow_chain: 4 * B * H * W * (2 n [4 n with the check] read + 2 (n+1) written)
 * + B * H * W * (n + 1 + 4) bytes; ofd_layer_composite: 4 * B * H * W * (n * (2 C + 2) + C + 1)). */
int ofd_flow_chain(const float* fwd, const float* bwd, float* disp, uint8_t* state, int32_t* life, int B, int T, int H, int W, int start,
                   int stop, int use_check, float a1, float a2, int all_steps, void* stream);
int ofd_flow_chain_to(const float* fwd, const float* bwd, float* disp, uint8_t* state, int B, int T, int H, int W, int anchor, int t0, int nt,
                      int use_check, float a1, float a2, void* stream);
int ofd_layer_composite(const float* frames, const float* layer, const float* disp, float* out, int B, int n, int C, int H, int W,
                        void* stream);

/* Motion-compensated temporal filtering: every pixel of a frame averaged with itself in the neighbouring frames, found by walking the
 * clip's flows from it (Liu & Freeman, "A high-quality video denoising algorithm based on reliable motion estimation", ECCV 2010; with
 * a guide that is not the filtered clip, the joint form of Lang et al., "Practical temporal consistency for image-based graphics
 * applications", SIGGRAPH 2012).  An addition: nothing in the reference looks at more than two frames.  One launch; the walks and the
 * sums stay in registers, no displacement and no gathered frame is stored.  All arithmetic fp32, every operation rounded on its own (no
 * contraction), in the order written; a chain without brackets runs left to right.
 * clip (B,T+1,C,H,W), 1 <= C <= 8: the values.  guide (B,T+1,Cg,H,W), 1 <= Cg <= 4, or NULL with Cg = 0: the clip guides itself, over its C
 * planes, and is read once.  fwd, bwd (B,T,2,H,W) in pixels with ofd_flow_chain's conventions, both non-null.  wt: HOST array of
 * radius + 1 floats, copied into the launch: wt[0] the centre's weight, wt[k] the weight of a tap k frames away; every one finite and
 * >= 0, not all zero (there is no exp on the device: warp.temporal_params makes them).  1 <= radius <= 8.  out (B,nt,C,H,W);
 * support (B,nt,1,H,W) fp32, the sum of the weights used; taps (B,nt,1,H,W) uint8, the neighbour taps that were used, 0..2*radius.  Slot
 * t - t0 holds frame t of [t0, t0 + nt).  For frame t and pixel p = (x, y):
 *   T1. Centre.  v0_c = clip[t]_c(p), g0_c = guide[t]_c(p) (the guide's planes; v0 itself without a guide).  If any of them is not
 *       finite: out = the centre's bits, support = +0.0, taps = 0, and both walks of the pixel are dead from the start (a dead walk
 *       reads offset 0 of a plane and drops what it reads).
 *   T2. Walks.  Two walks start at p with D = 0 and state 0: ahead over fwd[t], fwd[t+1], ..., step k arriving at frame t + k, for
 *       k = 1 .. min(radius, T - t); back over bwd[t-1], bwd[t-2], ..., step k arriving at frame t - k, for k = 1 .. min(radius, t).  A
 *       step is exactly ofd_flow_chain's: the same read of S at q, D' = D + v, the same states in the same order, and with use_check = 1
 *       the same read of K at q' and the same bound a1 * m + a2.  A dead walk stays dead and adds nothing further; no thread leaves the
 *       loop for it.
 *   T3. Tap.  After step k of a walk that is alive, q = ((float)x + D.x, (float)y + D.y) is inside the frame (the step would have left
 *       otherwise; the kernel tests it again before it forms an index).  One cell is formed at q, and the C value planes and the guide's
 *       planes of the frame arrived at are read with it by ofd_flow_chain's bilinear formula: val_c, gq_c (without a guide gq = val).
 *       If any of these is not finite -- a non-finite corner makes it so even under weight 0 -- the tap is dropped; the walk goes on.
 *   T4. Weight.  d2 = the sum over the guide's planes, in plane order from +0.0, of (gq_c - g0_c) * (gq_c - g0_c); with use_range = 0,
 *       d2 = +0.0 instead.  r = range_scale / (range_scale + d2), one correctly rounded division; the tap's weight is
 *       w = wt[k] * (r * r): ofd_motion_fit's Geman-McClure weight, and wt[k] exactly with use_range = 0.  range_scale is Cg * sigma_r^2
 *       (C * sigma_r^2 without a guide), finite and > 0.  (A finite gq so large that d2 overflows gives r = 0: the tap counts, with w = 0.)
 *   T5. Sums.  num_c = wt[0] * v0_c and den = wt[0]; then for every tap that was not dropped, the walk ahead k = 1, 2, ... first and
 *       the walk back k = 1, 2, ... after it: num_c = num_c + w * val_c, den = den + w, taps + 1.  out_c = num_c / den, support = den.
 *       Where den == 0 (wt[0] = 0 and no tap with w > 0), out = the centre's bits.
 *   T6. Aliasing and limits.  out, support and taps must not share a byte with clip, guide, fwd or bwd: a thread gathers other pixels'
 *       inputs.  H, W <= 32768; 1 <= T <= 4096; 0 <= t0, 1 <= nt, t0 + nt <= T + 1; a1, a2 finite and >= 0; use_range and use_check 0
 *       or 1; nt * B * ceil(H / 16) * ceil(W / 64) < 2^30; B * (T+1) * max(C, 2) * H * W < 2^40.  Every float becomes a gather index only
 *       after the inside test, which a non-finite or huge value fails: whatever the arrays hold, every read is inside its plane.
 * No atomics, no LDS, no host sync; a thread writes only its own pixels; the same input gives the same bits.  A workgroup owns a 64 x 16
 * tile of one frame and sample, so a frame's bits depend neither on how [t0, t0 + nt) is split over calls nor on what shares the
 * batch.  Argument errors return OFD_ERR_ARG and set ofd_last_error before any GPU work.  Per step and pixel a walk makes the chain's
 * 8 (16 with the check) corner loads and 4 * (C + Cg) more for the tap, each step's behind the one before: it is taken to be bound by
 * the latency of these gathers, like ofd_flow_chain.  Compulsory traffic: 4 * B * nt * H * W * (2 C + Cg + 1) + B * nt * H * W bytes plus the
 * flows of the frames it walks. */
int ofd_temporal_filter(const float* clip, const float* guide, const float* fwd, const float* bwd, const float* wt, float* out,
                        float* support, uint8_t* taps, int B, int T, int C, int Cg, int H, int W, int radius, int use_range,
                        float range_scale, int use_check, float a1, float a2, int t0, int nt, void* stream);

/* Flow-guided completion of a masked region of a clip: every hole pixel of a frame is followed through the clip's flows, ahead and back,
 * until it lands where another frame really saw the scene, and takes the colour there (Huang et al., "Temporally coherent completion
 * of dynamic video", SIGGRAPH Asia 2016; Xu et al., "Deep flow-guided video inpainting", CVPR 2019).  An addition: nothing in the
 * reference looks at more than two frames.  One launch; the walks stay in registers, no displacement and no gathered frame is stored.
 * All arithmetic fp32, every operation rounded on its own (no contraction), in the order written.
 * clip (B,T+1,C,H,W), 1 <= C <= 8.  mask (B,T+1,1,H,W) uint8: nonzero = hole, the pixels to be filled and never to be copied from.
 * fwd, bwd (B,T,2,H,W) in pixels with ofd_flow_chain's conventions, both non-null and already completed inside the holes (the flow
 * under a hole is the flow of what the hole hides: warp.complete_flows).  out (B,nt,C,H,W); steps (B,nt,2,H,W) uint8.  Slot t - t0
 * holds frame t of [t0, t0 + nt).  For frame t and pixel p = (x, y):
 *   F1. Non-hole pixel (mask[t](p) == 0).  out = the clip's bits, whatever they are; steps = (0, 0).
 *   F2. Walks.  For a hole pixel two walks start at p with D = 0 and state 0, exactly as in T2 of ofd_temporal_filter: ahead over
 *       fwd[t], fwd[t+1], ..., step k arriving at frame t + k, for k = 1 .. min(reach, T - t); back over bwd[t-1], bwd[t-2], ..., step k
 *       arriving at frame t - k, for k = 1 .. min(reach, t).  A step is exactly ofd_flow_chain's: the same read of S at q, D' = D + v,
 *       the same states in the same order, and with use_check = 1 the same read of K at q' and the same bound a1 * m + a2.  A dead walk
 *       stays dead.
 *   F3. Source.  After step k of a walk that is alive, q = ((float)x + D.x, (float)y + D.y) is inside the frame (the kernel tests it
 *       again before it forms an index).  One cell is formed at q: x0 = floor(q.x), x1 = min(x0 + 1, W-1), likewise in y.  The arrival is
 *       SEEN iff the four bytes of mask[t +- k] at (y0,x0), (y0,x1), (y1,x0), (y1,x1) are all 0 -- all four whatever their weights, so
 *       that a hole's colour can never enter a read; seen depends on the mask alone, not on what the clip holds.  The first seen arrival
 *       of a walk fixes its source: its k and its D.  From there on the walk is finished and adds nothing.
 *   F4. Colour.  For a walk with a source, val_c = the bilinear read of plane c of the frame arrived at, at that q, by ofd_flow_chain's
 *       formula.  A non-finite corner makes val_c non-finite even under weight 0: the caller can mask such pixels.  The colours are read
 *       once, after both walks, from the two stored D.
 *   F5. Result.  With k_f, k_b the steps of the sources ahead and back and vf, vb their colours: both found and blend = 1:
 *       a = (float)k_b, b = (float)k_f, out_c = (a * vf_c + b * vb_c) / (a + b) -- two products, their sum, the sum a + b, one division: the
 *       nearer source weighs more; both found and blend = 0: the walk with the smaller k wins, a tie goes to the walk ahead.  One found:
 *       its colour's bits.  Neither: the clip's own bits.  steps = (k_f, k_b), 0 = no source: the pixels still unfilled are those with
 *       mask != 0 and steps == (0, 0).
 *   F6. Aliasing and limits.  out and steps must not share a byte with clip, mask, fwd or bwd: a thread gathers other pixels' inputs.
 *       1 <= reach <= 255; H, W <= 32768; 1 <= T <= 4096; 0 <= t0, 1 <= nt, t0 + nt <= T + 1; a1, a2 finite and >= 0; use_check and blend
 *       0 or 1; nt * B * ceil(H / 16) * ceil(W / 64) < 2^30; B * (T+1) * max(C, 2) * H * W < 2^40.  Every float becomes a gather index only
 *       after the inside test, which a non-finite or huge value fails: whatever the arrays hold, every read is inside its plane.
 * No atomics, no LDS, no host sync; a thread writes only its own pixels; the same input gives the same bits.  A workgroup owns a 64 x 16
 * tile of one frame and sample, so a frame's bits depend neither on how [t0, t0 + nt) is split over calls nor on what shares the
 * batch.  The cost follows the hole, not the clip: a wave (64 columns of four rows) whose pixels hold no hole copies them and reads no
 * flow, and a wave leaves the step loop once every walk of its lanes is finished or dead; neither changes a bit.  Argument errors
 * return OFD_ERR_ARG and set ofd_last_error before any GPU work.  Per step and hole pixel a walk makes the chain's 8 (16 with the
 * check) corner loads and 4 byte loads of the mask, each step's behind the one before: it is taken to be bound by the latency of these
 * gathers, like ofd_flow_chain.  Compulsory traffic: B * nt * H * W * (8 C + 3) bytes plus the flows under the holes. */
int ofd_clip_fill(const float* clip, const uint8_t* mask, const float* fwd, const float* bwd, float* out, uint8_t* steps, int B, int T,
                  int C, int H, int W, int reach, int use_check, float a1, float a2, int blend, int t0, int nt, void* stream);

/* The membrane of a masked region: the solution of the discrete Laplace equation inside a hole, with the frame around the hole as
 * boundary data (the smooth interpolant that ofd_pushpull_fill approximates; added to a copied patch it is the guided interpolation of
 * Perez, Gangnet & Blake, "Poisson image editing", SIGGRAPH 2003).  An addition: nothing in the reference solves an equation.  A fixed
 * number of multigrid cycles, fixed in advance by the arguments: no convergence test and no host sync.  All arithmetic fp32, every
 * operation rounded on its own (no contraction), in the order written.
 * data (B,C,H,W), 1 <= C <= 8.  hole (B,1,H,W) uint8: nonzero = unknown (ofd_clip_fill's byte convention).  init (B,C,H,W) or NULL
 * (zeros): the start inside the hole.  out (B,C,H,W).  resid (B,) float.  cycles 1..32, nu 1..4, shape 1 (V) or 2 (W).
 *   M1. Effective hole.  A pixel is UNKNOWN iff its hole byte is nonzero or data is non-finite in any plane there (as in
 *       ofd_pushpull_fill); every other pixel is KNOWN.  At a known pixel out = data's bits.  data at an unknown pixel never reaches a
 *       result.  At an unknown pixel the solve starts from c = init (0 without init).
 *   M2. Levels.  Level 0 is the frame, H_0 x W_0 = H x W.  While H_l > 4 and W_l > 4 and l < 11 there is a level l + 1 of
 *       ceil(H_l / 2) x ceil(W_l / 2) cells; cell (Y, X) of it has the children (2Y, 2X), (2Y, 2X+1), (2Y+1, 2X), (2Y+1, 2X+1) of level l and
 *       is unknown iff all four are inside level l and unknown.  The number of levels follows from H and W alone -- a level without an
 *       unknown cell changes nothing, so the bits are those of stopping above it, except that the level above then makes its nu + nu
 *       sweeps and not M8's eight.  Per level and plane the state is c and b, read at unknown cells only.
 *   M3. Equation.  n_p = the number of 4-neighbours of p inside the level, as a float (the level's edge is a Neumann wall).
 *       S(t; p) = (t(x-1, y) + t(x+1, y)) + (t(x, y-1) + t(x, y+1)), a term outside the level being +0.0.  sum_p = S(c at unknown cells, +0.0
 *       elsewhere).  Level 0: b_p = S(data at known pixels, +0.0 elsewhere): a known pixel is Dirichlet data.  The equation at an unknown p
 *       is n_p * c_p - sum_p = b_p; on level l > 0, c is the error of level l - 1, b the restricted residual (M6), and a cell that is not
 *       unknown is error 0.
 *   M4. Sweep.  Red-black Gauss-Seidel: a sweep updates the unknown cells with ((x + y) & 1) == 0 in the level's own coordinates, then
 *       those with 1, by c_p = (b_p + sum_p) / n_p.  A cell's update reads cells of the other colour only, so within a colour the order
 *       of the cells does not matter, and sweeps fused in a tile with a halo have the bits of sweeps over the whole level.
 *   M5. Residual.  r_p = b_p - (n_p * c_p - sum_p) at an unknown cell.
 *   M6. Restriction.  At an unknown cell of level l + 1: b = (r(2Y, 2X) + r(2Y, 2X+1)) + (r(2Y+1, 2X) + r(2Y+1, 2X+1)), and c = 0.
 *   M7. Prolongation.  At an unknown cell (x, y) of level l: c = c + e, e = (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 +
 *       tx * v11): ofd_pushpull_fill's x2 bilinear read (half-pixel centres, weights 3/4 and 1/4, edge-clamped at the level's edge) of
 *       level l + 1's c, a cell of level l + 1 that is not unknown reading +0.0.  Per axis, i even: lo = max(i/2 - 1, 0), hi = i/2, t = 0.75;
 *       i odd: lo = i/2, hi = min(i/2 + 1, n - 1), t = 0.25; v00 = (y lo, x lo), v01 = (y lo, x hi), v10 = (y hi, x lo), v11 = (y hi, x hi).
 *   M8. Cycle of level l.  The last level: eight sweeps.  Otherwise nu sweeps; M5 and M6 (level l + 1's c restarts at 0); `shape`
 *       cycles of level l + 1, one after the other on the same c -- but level 0 descends once whatever `shape`; M7; nu sweeps.
 *       `cycles` cycles of level 0 are run.
 *   M9. Results.  out at unknown pixels = level 0's c.  resid[b] = the largest |r_p| (M5) over the unknown pixels and planes of sample
 *       b after the last cycle, 0 without unknown pixels; the maximum is taken on the bits of the non-negative floats as integers.
 *       A component of the hole that no known pixel touches solves a singular equation: it stays near its start.
 *   M10. Aliasing and limits.  out and resid must not share a byte with data, hole, init, the workspace or each other.  2 <= H, W <=
 *       32768; the last level has at most 4096 cells (a frame more than about a thousand times longer than wide is refused);
 *       B * C * H * W < 2^36; B * ceil(H / 16) * ceil(W / 64) < 2^30.
 * No float atomics.  The same input gives the same bits; a sample's bits depend neither on what shares its batch nor on how the level is
 * cut into tiles.  A workgroup owns a 64 x 16 tile of one level and sample and fuses the nu sweeps of a leg in LDS; a tile without an
 * unknown cell returns after reading its mask bytes: the cost follows the hole.  Every level of at most 4096 cells runs, with the
 * recursion under it, in one launch.  Argument errors (null pointers, C, cycles, nu, shape out of range, a short or misaligned workspace,
 * aliasing) return OFD_ERR_ARG and set ofd_last_error before any GPU work.
 * workspace: ofd_membrane_workspace(B,C,H,W) bytes (0 for a bad shape), 16-byte aligned. */
size_t ofd_membrane_workspace(int B, int C, int H, int W);
int ofd_membrane_solve(const float* data, const uint8_t* hole, const float* init, float* out, float* resid, int B, int C, int H, int W,
                       int cycles, int nu, int shape, void* workspace, size_t workspace_bytes, void* stream);

/* Global motion of a flow: a robust parametric fit of the motion most pixels share (the camera's), the split of a flow into that motion
 * and the rest, and the render of a frame through a homography (Odobez & Bouthemy 1995; Black & Anandan 1996).  An addition: the
 * reference treats a flow as one field.  flow: (B,2,H,W) in pixels, channel 0 = x, a pixel p of the frame moves to p + flow(p); conf:
 * (B,1,H,W) or NULL (every confidence 1).  All arithmetic of the fit and the field is double, every operation rounded on its own (no
 * contraction), in the order written here; brackets are as written and a chain without brackets runs left to right.
 *   M1. Coordinates.  cx = (W-1)/2, cy = (H-1)/2, s = max(W-1, H-1, 1)/2.  For the pixel (x, y) with the flow (u, v):
 *       xn = (x - cx)/s, yn = (y - cy)/s, un = u/s, vn = v/s.  The P = 2, 4, 6, 8 parameters p of model 0, 1, 2, 3 are in these
 *       coordinates; all-zero parameters are zero flow.
 *   M2. Model displacement (mu, mv) and denominator D at the parameters p:
 *       0 translation  mu = p0, mv = p1, D = 1.
 *       1 similarity   mu = (p0 + p2*xn) - p3*yn,  mv = (p1 + p3*xn) + p2*yn,  D = 1.
 *       2 affine       mu = (p0 + p2*xn) + p3*yn,  mv = (p1 + p4*xn) + p5*yn,  D = 1.
 *       3 homography   D = (1 + p6*xn) + p7*yn,  mu = (((xn + p0) + p2*xn) + p3*yn)/D - xn,  mv = (((yn + p1) + p4*xn) + p5*yn)/D - yn.
 *   M3. Design rows of a pixel, against un (Jx) and vn (Jy), with x' = xn + un, y' = yn + vn:
 *       homography  Jx = [1, 0, xn, yn, 0, 0, -(xn*x'), -(yn*x')],  Jy = [0, 1, 0, 0, xn, yn, -(xn*y'), -(yn*y')];
 *       affine      their first six entries;  similarity  Jx = [1, 0, xn, -yn], Jy = [0, 1, yn, xn];  translation  Jx = [1, 0], Jy = [0, 1].
 *       The 0 entries are static: a product with one of them is not formed.
 *   M4. Weight.  A pixel is usable when u, v and its confidence c are finite and c > 0; any other pixel has weight 0, is not counted and
 *       is not read further.  ex = (un - mu)*s, ey = (vn - mv)*s, r2 = ex*ex + ey*ey (pixels squared).  Solve 0: w = c.  Every later
 *       solve, at the parameters the solve before left: g = 1 + r2/(sigma*sigma), rho = 1/(g*g) (Geman-McClure), w = (c*rho)/(D*D).
 *       A usable pixel whose D is not > 0, or whose w or r2 is not finite, is counted and adds nothing else in that solve.
 *   M5. Sums.  Per sample and solve, over the usable pixels: a_ij = sum of (w*Jx[i])*Jx[j] + (w*Jy[i])*Jy[j] for i <= j (one product
 *       where the other is statically zero), b_i = sum of (w*Jx[i])*un + (w*Jy[i])*vn (likewise), sum w, sum w*r2, and the count
 *       (sum of 1.0): P(P+1)/2 + P + 3 values, 47 at P = 8.  Each is a double sum of the per-pixel terms in a fixed order: a thread adds its
 *       pixels' terms in ascending address from +0.0 (thread t of the sample's workgroup g takes the units g*256 + t, + wps*256, ...;
 *       a unit is 4 neighbouring pixels where H*W % 4 == 0 and flow and conf are 16-byte aligned, one pixel otherwise; a sample has
 *       wps = min(ceil(units / 256), 128) workgroups, a number that depends on the frame and the alignment and never on B), the workgroup's
 *       256 values go through the waves-then-four-slots order of ofd_nan_mse_rows' partials, and the partials g = 0, 1, ... are added
 *       in ascending order from +0.0.  No atomics, no float accumulation: the same input gives the same bits, run to run.  The order
 *       depends on the alignment; where every sum is exact it cannot matter.  It does not depend on B or on the sample's place in
 *       the call: a sample fitted alone, or in a chunk of a longer call, has the bits it has in the whole call, at the same alignment
 *       (which slices of one array share when H*W % 4 == 0).
 *   M6. Solve, of A p = b with A the symmetric matrix of the a_ij: the square-root-free Cholesky factorisation A = L diag(d) L^T (L unit
 *       lower triangular) and two triangular solves.  amax = the largest a_ii.  For j = 0 .. P-1: t_k = L[j][k]*d_k and
 *       d_j = a_jj - L[j][0]*t_0 - ... - L[j][j-1]*t_{j-1} (each product subtracted in turn, k ascending); the sample is DEGENERATE if
 *       d_j <= 1e-12 * amax or d_j is not finite; for i = j+1 .. P-1: L[i][j] = (a_ji - L[i][0]*t_0 - ... - L[i][j-1]*t_{j-1}) / d_j.
 *       Then z_i = b_i - L[i][0]*z_0 - ... - L[i][i-1]*z_{i-1} for i = 0 .. P-1; y_i = z_i / d_i; p_i = y_i - L[i+1][i]*p_{i+1} - ... -
 *       L[P-1][i]*p_{P-1} for i = P-1 .. 0.  A p with a non-finite entry is degenerate too.  (No square root: an integer translation
 *       on a frame whose s is a power of two is recovered exactly, whatever the weights sum to.)
 *   M7. ofd_motion_fit solves iterations + 1 times.  A degenerate solve leaves the sample's parameters what they were (zeros, the
 *       identity, if it is solve 0), and the sample stays degenerate for the remaining solves.  params (B,8): p, the unused tail 0.
 *       stats (B,4): sum w, sum w*r2 and the count of the LAST solve's sums (they describe the parameters that solve started from;
 *       with iterations = 0: zero parameters and w = c), and the status, 0 ok / 1 degenerate.
 *   M8. matrix (B,9), row-major 3x3, written after the last solve: M = N^-1 Hn N scaled to M[2][2] = 1, which maps [x, y, 1] to
 *       ~[x + u, y + v, 1] in pixels.  Hn = [[a, b, c], [d, e, f], [g, h, 1]] with c = p0, f = p1 and (a, b, d, e, g, h) =
 *       (1, 0, 0, 1, 0, 0) translation, (1 + p2, -p3, p3, 1 + p2, 0, 0) similarity, (1 + p2, p3, p4, 1 + p5, 0, 0) affine,
 *       (1 + p2, p3, p4, 1 + p5, p6, p7) homography.  gs = g/s, hs = h/s, k = 1 - (g*cx + h*cy)/s;
 *       M = [[a + cx*gs, b + cx*hs, (s*c - (a*cx + b*cy)) + cx*k], [d + cy*gs, e + cy*hs, (s*f - (d*cx + e*cy)) + cy*k], [gs, hs, k]],
 *       every entry then divided by k.  Zero parameters give the identity exactly.  If k is 0 or an entry is not finite, the matrix
 *       is the identity and the status 1.
 *   M9. A matrix M at the pixel (x, y): D = (M6*x + M7*y) + M8, X = ((M0*x + M1*y) + M2)/D, Y = ((M3*x + M4*y) + M5)/D, in double; the
 *       position is valid when D is finite and > 0.
 *       ofd_motion_field: model_flow = ((float)(X - x), (float)(Y - y)), NaN in both where the position is not valid.  residual =
 *       flow - model_flow, one fp32 subtraction; NaN propagates.  weight = (float)(c * rho) with rho of M4 from r2 = rx*rx + ry*ry of the
 *       fp32 residual taken in double; 0 where the residual or c is not finite or c <= 0.  flow == NULL (then conf, residual and
 *       weight must be NULL too) only synthesises the flow of the matrix.  One elementwise launch.
 *       ofd_homography_warp: img, out (B,C,H,W), 1 <= C <= 8; matrix maps an OUTPUT pixel to the source position (X, Y) it is read
 *       from; inside (B,1,H,W) or NULL.  Where the position is valid and 0 <= X <= W-1 and 0 <= Y <= H-1 (false for NaN): x0 = floor(X)
 *       in double, tx = (float)(X - x0), x1 = min(x0 + 1, W-1), likewise in y, and out_c = (1-ty) * ((1-tx) * g00 + tx * g01) + ty *
 *       ((1-tx) * g10 + tx * g11) in fp32, ofd_flow_chain's read; inside = 1.  Elsewhere out = +0.0 and inside = 0.  A position becomes
 *       an index only after that test; a pixel outside reads offset 0 of its plane and drops it.  One launch in ofd_layer_composite's
 *       tile and thread layout; no LDS, no atomics.
 * ofd_motion_fit enqueues 2 * (iterations + 1) launches and makes no host synchronisation; ws is ofd_motion_fit_ws_doubles(B, H, W)
 * doubles of device scratch, B * min(ceil(H*W / 256), 128) * 47: it grows with B, so the workspace of a call serves any call of
 * fewer samples.  H, W <= 32768; every array < 2^40 elements; model 0..3; 0 <= iterations <= 64; sigma finite and > 0;
 * outputs must not alias inputs or each other.  Argument errors return OFD_ERR_ARG and set ofd_last_error before any GPU work.  The fit
 * follows the majority: it breaks down as the outliers near half the weight, and a degenerate status is the only failure it reports
 * (several motions with no majority: ofd_motion_layers, below).
 * Compulsory traffic: the fit 4 * B * H * W * 2 (3 with conf) bytes per solve; the field 4 * B * H * W * (2 .. 8); the warp
 * 4 * B * H * W * (2 C + 1).  Measured (tools/motion_bench.py), no model's pass is bound by HBM: 1.8 TB/s (translation) to 0.5 TB/s
 * (homography) over these bytes at 16 x 440 x 1024. */
size_t ofd_motion_fit_ws_doubles(int B, int H, int W);
int ofd_motion_fit(const float* flow, const float* conf, int B, int H, int W, int model, int iterations, float sigma, double* params,
                   double* matrix, double* stats, double* ws, void* stream);
int ofd_motion_field(const double* matrix, const float* flow, const float* conf, float sigma, float* model_flow, float* residual,
                     float* weight, int B, int H, int W, void* stream);
int ofd_homography_warp(const float* img, const double* matrix, float* out, float* inside, int B, int C, int H, int W, void* stream);

/* Motion layers: the split of a flow into K parametric motions and the pixels that follow each (Wang & Adelson 1994; the multiple-
 * motions half of Black & Anandan 1996).  An addition: ofd_motion_fit describes ONE motion and follows the majority; a frame with a
 * camera and two objects, or a parallax scene with no majority, holds several.  flow, conf, the models, coordinates, design rows, a
 * pixel's weight and the arithmetic (double, every operation rounded on its own, in the order written) are M1 ... M4, unchanged.
 * Labels are uint8: 0 .. K-1 a layer, OFD_LABEL_OUTLIER = 254 (usable, no layer explains it), OFD_LABEL_INVALID = 255 (not usable).
 *   L1. Parameters.  1 <= K <= 8 layers; model 0..3; solves T, 0..64; sigma and tau (pixels) finite and > 0; min_support >= 1, raised
 *       to the model's parameter count P where it is below.  tau2 = tau*tau, sig2 = sigma*sigma, claim2 = (1.5*tau)*(1.5*tau), the
 *       floats taken in double first.  A pixel is usable as in M4; any other pixel is INVALID everywhere and is not read further.
 *   L2. Seeds, by peeling translations (in pixels, not normalised).  For k = 0 .. K-1 in turn: the candidates of layer k are the usable
 *       pixels with (u - tx_j)*(u - tx_j) + (v - ty_j)*(v - ty_j) > claim2 for every live j < k.  Eleven means follow; mean m sums, over
 *       the candidates, w*u, w*v, w and 1.0 with w = c in mean 0 and w = c * rho in mean 1 .. 10, rho of M4 from r2 = (u - tx_k)*(u - tx_k)
 *       + (v - ty_k)*(v - ty_k) and tau2 in sigma's place; then tx_k = (sum w*u) / (sum w), ty_k likewise.  The layer is DEAD if the
 *       count is < min_support, sum w is not finite and > 0, or a mean is not finite; it then stays dead, with zero parameters.  After
 *       mean 10: params = (tx_k / s, ty_k / s, 0, ...), exact for every model's parameterisation; matrix by M8; stats = (sum w, 0,
 *       count, status) of mean 10.  The sums are M5's: a thread adds its pixels' terms in ascending address from +0.0, the
 *       workgroup's values go through the waves-then-four-slots order, the partials are added in ascending order; units, workgroups
 *       per sample and the alignment rule are M5's.  The candidate test is evaluated from the earlier seeds on the fly.
 *   L3. T joint solves.  In each, every usable pixel evaluates r2_j and D_j (M2, M4) against every live layer's current parameters.  A
 *       layer whose D is not > 0 there, or whose r2 is not finite, cannot win the pixel; the pixel's label is the layer of least r2,
 *       the lowest index among equals; OUTLIER if no layer can win or the least r2 > tau2.  A pixel with label k adds 1.0 to layer
 *       k's count and, where w = (c * rho(r2_k)) / (D_k * D_k) is finite, M5's terms with that w to layer k's sums, in L2's order
 *       (the pixels of other labels add nothing).  Each live layer then gets M6's solve.  A layer whose count is < min_support, or
 *       whose solve is degenerate, keeps its parameters, is dead for every later solve and for ofd_motion_layers' status: 1.  stats
 *       (B,K,4): sum w, sum w*r2 and the count of the layer's LAST solve (zeros for a layer that was dead before it; with T = 0
 *       L2's), and the status, 0 live / 1 dead.  params (B,K,8) and matrix (B,K,9) as M7, M8, of every layer, dead ones too (the
 *       parameters it kept); a matrix that M8 cannot form is the identity and its layer dead.
 *   L4. Order.  ofd_motion_layers leaves the layers in seed order.  warp.segment_motion orders them by the last solve's count,
 *       descending, the lower index first among equals, dead layers last (a stable device sort and gathers: no kernel).
 *   L5. ofd_motion_assign, against pixel matrices (M9), one elementwise launch: for each layer j with alive[j] != 0 (all, if alive is
 *       NULL), (mx, my) = ((float)(X - x), (float)(Y - y)), (rx, ry) = (u - mx, v - my) in fp32, r2 = rx*rx + ry*ry with the fp32
 *       residual taken in double.  A layer whose position is not valid or whose r2 is not finite cannot win.  The label is the layer
 *       of least r2, the lowest index among equals; OUTLIER if none can win or the least r2 > tau2; INVALID where the pixel is not
 *       usable.  dist = (float)sqrt(r2) of the winner, model_flow and residual its (mx, my) and (rx, ry); all NaN where the label is
 *       OUTLIER or INVALID.  counts (B, K+2) int64: pixels per layer, then outliers, then invalid; zeroed by the call, integer atomics
 *       (a wave counts with ballots into its workgroup's table in LDS; one atomic per workgroup, sample and label).  With labels_in (B,1,H,W) the winner is not searched: a usable pixel takes the layer
 *       labels_in names if that layer is alive and can win there (no tau test), OUTLIER otherwise (also where labels_in is >= K); this
 *       recomputes dist, model_flow and residual for labels that ofd_label_vote changed.  Every output but labels may be NULL.
 *       The matrices may come from anywhere.  This assignment works from the rounded pixel matrices and the fp32 residual, L3 from
 *       the normalised parameters in double: at a pixel on a decision boundary (two layers equally near, or the winner at tau) the
 *       two may differ.
 *   L6. ofd_label_vote, radius 1..3, integer arithmetic only: a pixel takes the label 0 .. K-1 that is most frequent in its
 *       (2 radius + 1)^2 window, clipped to the frame; neighbours with any other label do not vote.  Among equally frequent labels
 *       the pixel's own wins if it is one of them, otherwise the lowest.  An OUTLIER pixel (any label >= K but INVALID) is filled
 *       where a neighbour votes; an INVALID pixel stays INVALID; a window without votes keeps the pixel's label.  A 64 x 16 tile per
 *       workgroup, the labels of the tile and its ring staged once in LDS.
 *   L7. ofd_motion_layers enqueues 2 * (11 K + T) launches and makes no host synchronisation; ws is ofd_motion_layers_ws_doubles(B, K,
 *       H, W) doubles of device scratch, B * K * (min(ceil(H*W / 256), 128) * 47 + 4).  In a joint solve a workgroup serves one (sample,
 *       share, layer): every pixel is read K times, and evaluated against the other layers only where its own is within tau.  A sample's bits do not depend on B or on what shares its call.
 * H, W <= 32768; every array < 2^40 elements; outputs must not alias inputs or each other.  Argument errors return OFD_ERR_ARG and set
 * ofd_last_error before any GPU work.  The seeds are translations: two motions that differ by less than 1.5 tau everywhere in the
 * frame share a seed.  tau, sigma, T, the claim radius 1.5 tau and the ten means come from synthetic band scenes; untuned on footage. */
#define OFD_LABEL_OUTLIER 254
#define OFD_LABEL_INVALID 255
size_t ofd_motion_layers_ws_doubles(int B, int K, int H, int W);
int ofd_motion_layers(const float* flow, const float* conf, int B, int H, int W, int model, int K, int solves, float sigma, float tau,
                      int min_support, double* params, double* matrix, double* stats, double* ws, void* stream);
int ofd_motion_assign(const double* matrix, const uint8_t* alive, const float* flow, const float* conf, float tau, const uint8_t* labels_in,
                      uint8_t* labels, float* dist, float* model_flow, float* residual, int64_t* counts, int B, int K, int H, int W,
                      void* stream);
int ofd_label_vote(const uint8_t* labels, uint8_t* out, int B, int H, int W, int K, int radius, void* stream);

/* Background plate of a clip: the frames gathered through their camera path into one coordinate system and reduced over time, and the
 * plate read back into every frame (Wang & Adelson 1994: a layer's intensity map is the temporal median of the warped frames; Irani,
 * Anandan & Hsu 1995: mosaics of a pan).  An addition: ofd_homography_warp renders one frame at its own size and keeps what moves.
 * Every operation is rounded on its own (no contraction), in the order written; a chain without brackets runs left to right.
 *   P1. ofd_plate_reduce, arguments.  clip (B,N,C,H,W) fp32, 1 <= C <= 8, 1 <= N <= OFD_PLATE_MAX_FRAMES; weight (B,N,1,H,W) fp32 or NULL
 *       (every weight 1); path (B,N,9) double, path[b][t] sends an anchor position to the place in frame t it is read from (what
 *       warp.camera_path(mode="lock") returns); plate (B,C,Hc,Wc) fp32; votes (B,1,Hc,Wc) fp32 or NULL; count (B,1,Hc,Wc) uint8 or NULL.
 *       The canvas pixel (i, j) (column, row) stands at the anchor position (x, y) = ((double)(x0 + i), (double)(y0 + j)); x0, y0 ints
 *       with |x0|, |y0| <= 32768.  mode 0 median, 1 mean; 1 <= min_count <= N.
 *   P2. The sample of frame t at a canvas pixel.  (X, Y) = path[b][t] at (x, y) by M9.  Valid and inside are tested as in
 *       ofd_homography_warp (D finite and > 0, 0 <= X <= W-1, 0 <= Y <= H-1 in double, false for NaN); the cell (x0 = floor(X) in double,
 *       tx = (float)(X - x0), x1 = min(x0 + 1, W-1), likewise in y) and the fp32 blend (1-ty) * ((1-tx) * g00 + tx * g01) + ty *
 *       ((1-tx) * g10 + tx * g11) are as written there.  v[t][c] is the blend of plane c of frame t; w[t] the blend of the weight
 *       plane, or 1.0f when weight is NULL.  The sample is usable when the position is valid and inside, w[t] is finite and > 0, and
 *       all C values v[t][c] are finite.  A position becomes an index only after the inside test; a sample outside reads offset 0 of
 *       its planes and drops it.
 *   P3. Quantised weight, fp32 left to right: q[t] = (uint32) floorf(fminf(w[t], 1.0f) * 65535.0f + 0.5f); a sample with q[t] = 0 is
 *       not usable.  Q = sum of q[t] and n = the number of usable samples (integer sums: no order).  votes = (float)Q / 65535.0f;
 *       count = n.
 *   P4. When n < min_count or Q = 0: plate = +0.0 in every plane.
 *   P5. mode 0, the lower weighted median, for each plane c by itself.  Order the usable samples by (v[t][c] ascending, t ascending)
 *       under the float `<` (-0.0 and +0.0 tie, and t decides); below_k = the sum of q over the samples before k; plate_c = the bits of
 *       v[k][c] at the one sample with 2 * below_k < Q <= 2 * (below_k + q[k]).  It is always one of the N samples.  Found by counting,
 *       not by sorting.
 *   P6. mode 1, the weighted mean: plate_c = (float)(S / (double)Q), S = the sum over the usable t, ascending from +0.0, of
 *       (double)q[t] * (double)v[t][c] in double.
 *   P7. ofd_plate_project, arguments and read.  plate (B,C,Hc,Wc); votes (B,1,Hc,Wc) or NULL; inv (B,N,9) double, inv[b][t] sends the
 *       pixel (x, y) of frame t to its anchor position (X, Y) by M9; any N >= 1.  The canvas position is (X - x0, Y - y0), double
 *       subtractions.  A pixel is covered when the position is valid, 0 <= X - x0 <= Wc-1 and 0 <= Y - y0 <= Hc-1 (false for NaN), and,
 *       where votes is given, the votes at all four corner texels of the cell are > 0.  proj_c is the fp32 blend of P2 on plane c of
 *       the plate.  covered (B,N,1,H,W) fp32 or NULL holds 1 or 0.  A pixel whose position fails the test reads offset 0 and drops it.
 *   P8. Output, out (B,N,C,H,W).  frames NULL (then alpha and fg must be NULL): out_c = proj_c where the pixel is covered, +0.0
 *       elsewhere.  frames (B,N,C,H,W) given: d = (|frame_0 - proj_0| + |frame_1 - proj_1| + ...) / (float)C in fp32, c ascending.
 *       With alpha (B,N,1,H,W): a = fminf(fmaxf(alpha, 0), 1), and 0 where alpha is not finite.  Otherwise a = fminf(fmaxf((d - lo) /
 *       (hi - lo), 0), 1) with 0 <= lo < hi finite, and 0 where d is NaN.  Where the pixel is not covered a = 0.  out_c = the bits of
 *       frame_c where a == 0, the bits of proj_c where a == 1, frame_c + a * (proj_c - frame_c) elsewhere: because of the two selects a
 *       non-finite value on the side that is not chosen never leaks.  fg (B,N,1,H,W) or NULL holds a.
 * Each entry point is one launch, makes no host synchronisation and uses no atomics; no float becomes an index before it passed the
 * inside test; the same input gives the same bits; a sample's bits do not depend on B or on what shares its call.  H, W, Hc, Wc <= 32768;
 * every array < 2^40 elements; outputs must not overlap inputs or each other.  Argument errors return OFD_ERR_ARG and set
 * ofd_last_error before any GPU work.  Nothing is inpainted: where no frame saw the background, votes is 0 and the plate +0.0.
 * Compulsory traffic: the reduce 4 * B * (N * (C + 1) * H * W + (C + 1) * Hc * Wc) + B * Hc * Wc bytes (the weight and votes planes
 * included); the projection 4 * B * N * H * W * (2 C + 2) bytes plus the plate.  Measured (tools/plate_bench.py) at 16 x 3 x 440 x 1024:
 * the median 1.7 TB/s (N = 8) and 0.66 TB/s (N = 32) over these bytes, the projection 2.4 TB/s. */
#define OFD_PLATE_MAX_FRAMES 32
int ofd_plate_reduce(const float* clip, const float* weight, const double* path, float* plate, float* votes, uint8_t* count, int B, int N,
                     int C, int H, int W, int x0, int y0, int Hc, int Wc, int mode, int min_count, void* stream);
int ofd_plate_project(const float* plate, const float* votes, const double* inv, const float* frames, const float* alpha, float* out,
                      float* covered, float* fg, int B, int N, int C, int H, int W, int x0, int y0, int Hc, int Wc, float lo, float hi,
                      void* stream);

/* ------------------------------------------------------------ grid_sample warp (WP:95-119) -
 * second: (B,C,H,W), flow: (B,2,H,W) exactly as handed to the reference's warp(mode='backward'):
 * after its flip(1) channel 1 displaces x and channel 0 displaces y (WP:105-106).
 * out, mask: (B,C,H,W); mask may be NULL.  bilinear, zeros padding, align_corners=True. */
int ofd_grid_warp_fwd(const float* second, const float* flow, float* out, float* mask,
                      int B, int C, int H, int W, void* stream);
/* Backward of the call above (what autograd derives for WP:95-119; the thresholded mask has no gradient).
 * grad_second (B,C,H,W): bilinear scatter of grad_out to the forward's four corners (the splat kernel on grid_sample's
 *   coordinates; needs a workspace of ofd_splat_workspace_bytes(B,H,W); radius as in ofd_splat_fwd, >= the largest |flow|
 *   keeps the far-corner list empty).  NULL: skipped.
 * grad_flow (B,2,H,W): ATen's grid gradient chained through the reference's normalisation (its (W-1)/2 and 2/(W-1) factors
 *   are applied in the reference's order); channel 1 receives d/dx.  NULL: skipped (second may then be NULL). */
int ofd_grid_warp_bwd(const float* second, const float* flow, const float* grad_out, float* grad_second, float* grad_flow,
                      int B, int C, int H, int W, int radius, void* workspace, size_t workspace_bytes, void* stream);
/* integer north-west corner (ix_nw, iy_nw) per pixel, int32 (B,H,W,2): index parity tests. */
int ofd_grid_warp_corners(const float* flow, int32_t* corners, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------- diffusion elementwise -
 * x_t, model_out, noise, out: (B,C,H,W) fp32 with n_per_sample = C*H*W.  Coefficients are
 * per-sample fp32 arrays of length B gathered by the host from the schedule (DD:422-425). */
int ofd_q_sample(const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac,
                 float* out, int B, size_t n_per_sample, void* stream);
/* x_{t-1} = c1*clamp(model_out) + c2*x_t + sigma*noise (sigma = exp(0.5*logvar); pass noise=NULL
 * or sigma=0 at t == 0).  x_start (clamped model_out) is written when non-NULL. */
int ofd_ddpm_update(const float* x_t, const float* model_out, const float* noise,
                    const float* coef1, const float* coef2, const float* sigma,
                    float* out, float* x_start, int B, size_t n_per_sample, void* stream);
/* DDIM (DD:750-767): x0 = clamp(model_out); eps = (sr*x_t - x0)/srm1;
 * out = x0*sqrt_an + c*eps + sigma*noise; last != 0 returns x0. */
int ofd_ddim_update(const float* x_t, const float* model_out, const float* noise,
                    const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                    const float* sqrt_alpha_next, const float* c, const float* sigma, int last,
                    float* out, float* x_start, int B, size_t n_per_sample, void* stream);
/* The objective-aware forms (DD:589-611, 634-664).  objective: OFD_PRED_X0, OFD_PRED_NOISE or OFD_PRED_V.  x_start before the
 * clamp is model_out (pred_x0), xa*x_t - xb*model_out with (xa, xb) = (sqrt_recip_ac, sqrt_recipm1_ac) for pred_noise and
 * (sqrt_ac, sqrt_1mac) for pred_v; xa / xb may be NULL for pred_x0.  The DDPM step clamps it (DD:670-671); the DDIM step clamps it
 * and re-derives eps from the clamped value for every objective (clip_x_start, rederive_pred_noise, DD:645-662).  Each product is
 * rounded on its own (no FMA contraction), as torch computes it.  ofd_q_sample / ofd_ddpm_update / ofd_ddim_update are the
 * OFD_PRED_X0 instantiations. */
#define OFD_PRED_X0 0
#define OFD_PRED_NOISE 1
#define OFD_PRED_V 2
int ofd_ddpm_update_obj(int objective, const float* x_t, const float* model_out, const float* noise,
                        const float* coef1, const float* coef2, const float* sigma, const float* xa, const float* xb,
                        float* out, float* x_start, int B, size_t n_per_sample, void* stream);
int ofd_ddim_update_obj(int objective, const float* x_t, const float* model_out, const float* noise,
                        const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* xa, const float* xb,
                        const float* sqrt_alpha_next, const float* c, const float* sigma, int last,
                        float* out, float* x_start, int B, size_t n_per_sample, void* stream);
/* DPM-Solver++ multistep step (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", 2022,
 * data prediction; an addition, not the reference's sampler).  With alpha = sqrt(ac), sigma = sqrt(1 - ac), lambda = log(alpha/sigma),
 * h = lambda_next - lambda_cur and D_k the clamped x_start predictions of this (k = 0) and the previous k steps:
 *   order 1: x_next = (sigma_next/sigma_cur) x_t - alpha_next*expm1(-h)*D0                    (= DDIM with eta = 0)
 *   order 2 (2M, paper Alg. 2): ... - alpha_next*expm1(-h)*(D0 + (D0 - D1)/(2r)),  r = h_prev/h
 *   order 3 (3M): ... + alpha_next*(expm1(-h)/h + 1)*D1' - alpha_next*((expm1(-h) + h)/h^2 - 1/2)*D2'  with the divided differences
 *            D1' = d0 + r0/(r0 + r1)*(d0 - d1), D2' = (d0 - d1)/(r0 + r1), d0 = (D0 - D1)/r0, d1 = (D1 - D2)/r1.
 * The host folds each into per-sample rows: out = cx*x_t + w0*D0 + w1*d_prev1 + w2*d_prev2 (order 1 reads no history, order 2
 * d_prev1 and w1, order 3 also d_prev2 and w2; each product rounded once, added in that order).  D0 = clamp(x_start, -1, 1) with
 * x_start formed as in ofd_ddim_update_obj (xa / xb as there, NULL for OFD_PRED_X0).  last != 0 writes D0 to out (the final
 * evaluation; no coefficient or history is read).  D0 is also written to d_out when non-NULL.  out == x_t is allowed. */
int ofd_dpmpp_update(int objective, int order, const float* x_t, const float* model_out, const float* xa, const float* xb,
                     const float* d_prev1, const float* d_prev2, const float* cx, const float* w0, const float* w1,
                     const float* w2, int last, float* out, float* d_out, int B, size_t n_per_sample, void* stream);
/* Constrained sampling: the three reverse steps with part of the diffused tensor held at known values (replacement-based inpainting:
 * Lugmayr et al., "RePaint", 2022; the imputation sampler of Song et al., "Score-Based Generative Modeling through SDEs", 2021; an
 * addition, not in the reference).  The arguments are those of ofd_ddpm_update_obj / ofd_ddim_update_obj / ofd_dpmpp_update, plus
 *   known           (B,C,H,W): a NaN element is FREE, any other is HELD at clamp(known, -1, 1); the mask is per element;
 *   e0              (B,C,H,W): x_T, the start of the chain, read only by a step that has no noise of its own (NULL otherwise);
 *                   it must outlive the chain: no step may write it;
 *   sqrt_ac_next, sqrt_1mac_next  per-sample sqrt(ac_s), sqrt(1 - ac_s) of the level s the step goes TO; NULL on the final step
 *                   (for the DDPM form, which has no `last`, NULL is what marks the final step, t = 0).
 * For a step from level t to level s:
 *   1. x_start (D0) is formed and clamped as in the unconstrained call, then overwritten by clamp(known) at held elements, before
 *      it is written to x_start / d_out (so a multistep history's divided differences are exactly zero there);
 *   2. free elements of out are the same bits the unconstrained entry point writes for the same inputs (the same device code);
 *   3. held elements of out are sqrt_ac_next*clamp(known) + sqrt_1mac_next*e, each product rounded on its own, where e is the
 *      element of `noise` when noise is non-NULL (the sampler drew noise at this step, whatever sigma is) and of e0 otherwise: a held
 *      element then follows the deterministic trajectory of a point mass at known;
 *   4. the final step writes clamp(known) itself at held elements.
 * Same access pattern as the unconstrained kernels: one 16-byte access per operand when n_per_sample % 4 == 0, one dword otherwise;
 * 4 reads (x_t, model_out, known, noise or e0) and up to 2 writes per element, plus the histories of the DPM-Solver++ form; out == x_t
 * stays allowed there.  One launch, no atomics. */
int ofd_ddpm_update_known(int objective, const float* x_t, const float* model_out, const float* noise,
                          const float* coef1, const float* coef2, const float* sigma, const float* xa, const float* xb,
                          const float* known, const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next,
                          float* out, float* x_start, int B, size_t n_per_sample, void* stream);
int ofd_ddim_update_known(int objective, const float* x_t, const float* model_out, const float* noise,
                          const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* xa, const float* xb,
                          const float* sqrt_alpha_next, const float* c, const float* sigma, int last,
                          const float* known, const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next,
                          float* out, float* x_start, int B, size_t n_per_sample, void* stream);
int ofd_dpmpp_update_known(int objective, int order, const float* x_t, const float* model_out, const float* xa, const float* xb,
                           const float* d_prev1, const float* d_prev2, const float* cx, const float* w0, const float* w1,
                           const float* w2, int last, const float* known, const float* e0, const float* sqrt_ac_next,
                           const float* sqrt_1mac_next, float* out, float* d_out, int B, size_t n_per_sample, void* stream);
/* Classifier-free guidance (Ho & Salimans, "Classifier-Free Diffusion Guidance", 2022; an addition, not in the reference): the three
 * reverse steps on two model outputs, the one of the condition (model_out) and the one of the null condition (model_out_uncond, with
 * the layout of model_out).  The arguments are those of the _known entry points, plus, after model_out,
 *   model_out_uncond  (B,C,H,W);
 *   guidance          per-sample scale w, B floats like every other coefficient row: 0 = unconditional, 1 = conditional, > 1 extrapolates.
 * known == NULL is the unconstrained step; e0, sqrt_ac_next and sqrt_1mac_next must then be NULL too.  Otherwise the constraint
 * composes with the guidance.
 *   G1. Per element m = u + w*(c - u) in fp32 (c of model_out, u of model_out_uncond, w = guidance[sample]; the product and both sums
 *       rounded on their own), except that w == 0 gives u itself.  m is formed in registers and used wherever the unguided step uses
 *       the model output: it goes through the objective's x_start formula and then the clamp.  eps, x0 and v are affine in each other
 *       given x_t, so guiding the raw output is the same guidance for every objective.  No intermediate tensor is written: one launch,
 *       reading one tensor more than the sibling (4 B per element).
 *   G2. A guidance row of zeros gives the bits of the unguided entry point called on model_out_uncond (out, x_start, d_out), and
 *       model_out is then not used (a NaN there does not reach the output).
 *   G3. With known, held elements are the bits of the _known entry point (they do not depend on the model output); free elements are
 *       the bits of the guided call without known.
 *   G4. out == x_t stays allowed for the DPM-Solver++ form, with the same bits as out of place.
 *   G5. Argument errors (a NULL model_out_uncond or guidance, constrained-only arguments without known, and everything the siblings
 *       refuse) return an error and set ofd_last_error before any GPU work. */
int ofd_ddpm_update_guided(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                           const float* guidance, const float* noise, const float* coef1, const float* coef2, const float* sigma,
                           const float* xa, const float* xb, const float* known, const float* e0, const float* sqrt_ac_next,
                           const float* sqrt_1mac_next, float* out, float* x_start, int B, size_t n_per_sample, void* stream);
int ofd_ddim_update_guided(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                           const float* guidance, const float* noise, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac,
                           const float* xa, const float* xb, const float* sqrt_alpha_next, const float* c, const float* sigma, int last,
                           const float* known, const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next,
                           float* out, float* x_start, int B, size_t n_per_sample, void* stream);
int ofd_dpmpp_update_guided(int objective, int order, const float* x_t, const float* model_out, const float* model_out_uncond,
                            const float* guidance, const float* xa, const float* xb, const float* d_prev1, const float* d_prev2,
                            const float* cx, const float* w0, const float* w1, const float* w2, int last, const float* known,
                            const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out, float* d_out,
                            int B, size_t n_per_sample, void* stream);
/* Dynamic thresholding (Saharia et al., "Photorealistic Text-to-Image Diffusion Models with Deep Language Understanding", 2022, section
 * 2.3; an addition, not in the reference): instead of the static clamp to [-1, 1], x_start is clamped to [-s, s] and divided by s, with
 * s a per-sample order statistic of |x_start|, raised to at least 1.  Two pieces: the statistic, and the three reverse steps reading it.
 *
 * ofd_x0_abs_quantile: thresh[b] = min(max(q_b, 1), max_value), q_b the rank-th smallest |x_start| over sample b's n_per_sample
 * elements (1 <= rank <= n_per_sample; an exact order statistic, no interpolation, no histogram approximation).  x_start is the
 * UNCLAMPED value the step forms from the same arguments: model_out (pred_x0) or xa*x_t - xb*model_out, with model_out replaced by the
 * guided combination G1 when model_out_uncond / guidance are given (both, or both NULL) -- the same device functions as the steps,
 * each product rounded on its own, so the value ranked is the value the step clamps.  x_t, xa and xb may be NULL for OFD_PRED_X0.  A
 * non-finite magnitude ranks above every finite one (Inf below NaN); a non-finite q_b gives max_value (finite, >= 1), so the row is
 * always finite and >= 1.  Elements a constrained step holds are not excluded: the statistic is over the model's prediction.
 * The bits of a non-negative float are monotone as an unsigned integer, so the selection is a radix select over the bits of |x_start|:
 * three passes of 11 / 11 / 10 bits, each one launch that counts digits (per-workgroup LDS histograms, merged into a (B, 2048) histogram
 * with integer atomics) and one small launch per pass that picks the digit and leaves the prefix and the remaining rank in the
 * workspace for the next pass.  Every pass re-forms x_start (4 to 12 B read per element and pass); nothing tensor-sized is written.  No
 * host synchronisation, no float atomics: the same inputs give the same bits.  workspace: ofd_x0_abs_quantile_ws_bytes(B) bytes,
 * 4-byte aligned, contents irrelevant on entry.  n_per_sample < 2^32. */
size_t ofd_x0_abs_quantile_ws_bytes(int B);
int ofd_x0_abs_quantile(int objective, const float* x_t, const float* model_out, const float* model_out_uncond, const float* guidance,
                        const float* xa, const float* xb, int B, size_t n_per_sample, size_t rank, float max_value, float* thresh,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The thresholded reverse steps.  The arguments are those of the _guided entry points plus, after guidance,
 *   thresh            per-sample threshold s, B floats, s >= 1 (what ofd_x0_abs_quantile writes).
 * model_out_uncond and guidance are both NULL for an unguided step; known, e0, sqrt_ac_next and sqrt_1mac_next are all NULL for an
 * unconstrained one.
 *   T1. The x_start of a free element is clamp(x, -s, s) / s (the division correctly rounded) with x exactly the unclamped value the
 *       sibling clamps to [-1, 1]; it is what the posterior mean, the DDIM eps re-derivation and the DPM-Solver++ update use, and what is
 *       written to x_start / d_out.  Nothing else changes.
 *   T2. A row of ones gives the bits of the corresponding sibling (plain, _known, _guided, _guided with known) for out, x_start and
 *       d_out.
 *   T3. Held elements are the bits of the _known entry point: clamp(known, -1, 1), not thresholded.
 *   T4. out == x_t stays allowed for the DPM-Solver++ form, with the same bits as out of place.
 *   T5. Argument errors (a NULL thresh, model_out_uncond without guidance or the reverse, and everything the siblings refuse) return
 *       an error and set ofd_last_error before any GPU work. */
int ofd_ddpm_update_thresh(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                           const float* guidance, const float* thresh, const float* noise, const float* coef1, const float* coef2,
                           const float* sigma, const float* xa, const float* xb, const float* known, const float* e0,
                           const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out, float* x_start, int B,
                           size_t n_per_sample, void* stream);
int ofd_ddim_update_thresh(int objective, const float* x_t, const float* model_out, const float* model_out_uncond,
                           const float* guidance, const float* thresh, const float* noise, const float* sqrt_recip_ac,
                           const float* sqrt_recipm1_ac, const float* xa, const float* xb, const float* sqrt_alpha_next, const float* c,
                           const float* sigma, int last, const float* known, const float* e0, const float* sqrt_ac_next,
                           const float* sqrt_1mac_next, float* out, float* x_start, int B, size_t n_per_sample, void* stream);
int ofd_dpmpp_update_thresh(int objective, int order, const float* x_t, const float* model_out, const float* model_out_uncond,
                            const float* guidance, const float* thresh, const float* xa, const float* xb, const float* d_prev1,
                            const float* d_prev2, const float* cx, const float* w0, const float* w1, const float* w2, int last,
                            const float* known, const float* e0, const float* sqrt_ac_next, const float* sqrt_1mac_next, float* out,
                            float* d_out, int B, size_t n_per_sample, void* stream);
/* Photometric guidance (an addition, not in the reference): one optional launch per reverse step that rewrites the model output so that
 * the predicted flow moves one damped Gauss-Newton step (Lucas & Kanade 1981; Levenberg 1944 / Marquardt 1963 damping) towards
 * photometric agreement of two frames, first(p) ~ second(p + f(p)).  It acts on the predicted x_start alone, as manifold-preserving
 * guided diffusion does (He et al. 2024); nothing is differentiated through the network (cf. Chung et al. 2023).  Every reverse step,
 * the quantile and the guided combination read the model output only, so they compose with it unchanged.
 *
 * The pyramid.  levels: HOST array of n_levels (1..4) positive integers L, each dividing H and W, read at call time.  Level k of a
 * (B, Ci, H, W) fp32 frame is its L_k x L_k box average, a contiguous (B, Ci, H / L_k, W / L_k) fp32 block; the blocks are packed in
 * the order of `levels`, ofd_photo_pyramid_floats(...) floats in all (0 for bad arguments).  ofd_photo_pyramid builds it, one launch
 * per level; it is meant to run once per chain and frame.  The step gathers both frames from these packed pyramids; no full-resolution
 * copy of the first frame's samples is kept.
 *
 * The step, per sample b and pixel p = (x, y), all in fp32:
 *   x0     the unclamped x_start of the flow channels c0, c0 + 1 of the (B, C, H, W) diffused tensor, formed exactly as the reverse
 *          steps form it: model_out (pred_x0) or xa*x_t - xb*model_out, with model_out replaced by the guided combination G1 when
 *          model_out_uncond / guidance are given.  x_t, xa and xb are NULL for OFD_PRED_X0 and required otherwise.
 *   f      = flow_max * clamp(x0, -1, 1), in pixels; channel c0 displaces x, channel c0 + 1 displaces y (the forward splat's order).
 *   A full-resolution coordinate u is (u + 0.5) / L - 0.5 at level L.  a_{L,c}: the bilinear sample of first_L at p's own level
 *   coordinate, clamped to the image.  b_{L,c}: the bilinear sample of second_L at the level coordinate of p + f; a level where that
 *   coordinate lies outside [0, W/L - 1] x [0, H/L - 1] contributes nothing at p.  r = b - a; J = db/df, the derivative of the bilinear
 *   interpolant inside its cell (the cell of floor(coordinate), the last cell at the far edge) over L.
 *   A = sum J J^T + damping I,  g = sum J r  (sums over levels and the Ci channels),  delta = -A^-1 g  (closed 2x2 solve),
 *   dx0 = step[b] * delta / flow_max.
 * Written back: pred_x0: out = model_out + dx0; pred_noise / pred_v: out = model_out - dx0 / xb[b], unchanged where xb[b] == 0.  With
 * the uncond pair the same increment goes to out and out_uncond (their guided combination moves by exactly that increment for any w).
 * Bit for bit unchanged: a pixel whose x0 is non-finite in either flow channel, a sample whose step[b] == 0, every channel outside
 * c0, c0 + 1.  out may be model_out and out_uncond may be model_out_uncond (a pixel reads and writes only itself); when they differ
 * the untouched values are copied through.  model_out_uncond, guidance and out_uncond come together or not at all.  One pixel per
 * thread in a grid-stride loop; no atomics, no host synchronisation: the same inputs give the same bits.  Ci 1..4, c0 + 2 <= C,
 * flow_max and damping finite and > 0.  Argument errors return OFD_ERR_ARG and set ofd_last_error before any GPU work. */
size_t ofd_photo_pyramid_floats(int B, int Ci, int H, int W, const int* levels, int n_levels);
int ofd_photo_pyramid(const float* img, const int* levels, int n_levels, int B, int Ci, int H, int W, float* pyr, void* stream);
int ofd_photo_guide(int objective, const float* x_t, const float* model_out, const float* model_out_uncond, const float* guidance,
                    const float* xa, const float* xb, const float* step, const float* first_pyr, const float* second_pyr,
                    const int* levels, int n_levels, int B, int C, int c0, int Ci, int H, int W, float flow_max, float damping,
                    float* out, float* out_uncond, void* stream);
/* Training prep, one launch (DD:844-848, 806-812, 874-879, 985-993), x0 / noise / outputs (B,C,hw):
 *   x0n = normalize ? 2*x0 - 1 : x0;  nz = noise + offset_strength*offset[b,c] (offset (B,C), or NULL: no offset noise);
 *   x_t = sqrt_ac*x0n + sqrt_1mac*nz;  target = nz (pred_noise), x0n (pred_x0), sqrt_ac*nz - sqrt_1mac*x0n (pred_v).
 * target and x_norm (x0n) are written when non-NULL; noise is never modified. */
int ofd_diffusion_prep(int objective, const float* x0, const float* noise, const float* offset, float offset_strength,
                       const float* sqrt_ac, const float* sqrt_1mac, int normalize, float* x_t, float* target, float* x_norm,
                       int B, int C, size_t hw, void* stream);
/* DD:73-77 over n floats: mode 0 -> 2*in - 1 (normalize), mode 1 -> (in + 1)*0.5 (unnormalize); in == out allowed. */
int ofd_range_map(const float* in, float* out, size_t n, int mode, void* stream);
/* Condition dropout of classifier-free guidance training (not in the reference), cond / out (B, n_per_sample), keep B floats:
 * a sample with keep != 0 gets exactly what ofd_range_map(mode) writes (the same bits); a sample with keep == 0 gets +0.0 everywhere,
 * whatever cond holds there (it is not read: a NaN or Inf cannot leak).  mode: ofd_range_map's 0 / 1, or OFD_COND_COPY (no mapping, for
 * a condition that is already in the model's range).  One pass, one launch; cond == out is not allowed. */
#define OFD_COND_COPY 2
int ofd_cond_drop(const float* cond, const float* keep, int mode, float* out, int B, size_t n_per_sample, void* stream);
/* sum and count over positions where neither pred nor target is NaN of (pred-target)^2.
 * result (device): ofd_nan_mse_result_doubles() doubles -- [0] sum, [1] count, the rest scratch (per-workgroup partial sums, added
 * in a fixed order: the same inputs give the same sum bit for bit). */
size_t ofd_nan_mse_result_doubles(void);
int ofd_nan_mse_sum(const float* pred, const float* target, size_t n, double* result, void* stream);
/* backward of result[0] / result[1] (the nanmean): dpred = 2 (pred - target) * gout[0] / result[1] on finite pairs, else 0;
 * result is what ofd_nan_mse_sum left, gout a device scalar */
int ofd_nan_mse_grad(const float* pred, const float* target, size_t n, const double* result, const float* gout,
                     float* dpred, void* stream);
/* The same reduction per sample, for a per-sample loss weight (min-SNR weighting, Hang et al., "Efficient Diffusion Training via Min-SNR
 * Weighting Strategy", 2023; an addition: the reference builds the weight table and leaves it unused, DD:975-980).  pred / target are
 * contiguous (B, n_per_sample); weight is B floats on the device, or NULL; result is ofd_nan_mse_rows_result_doubles(B) doubles.
 *   R1. result[2 + 2b] = S_b, the sum over sample b of (float)(p - t) squared in fp32, over the elements where neither side is NaN,
 *       accumulated in double; result[3 + 2b] = N_b, the number of such elements.  A sample with no such element has S_b = 0, N_b = 0.
 *   R2. result[0] = sum_b (double)weight[b] * S_b, added in ascending b; result[1] = sum_b N_b.  weight == NULL means every weight is 1.
 *       The rest of result is scratch.
 *   R3. No float atomics and a fixed summation order: the same inputs give the same bits in every element of result[0 .. 2 + 2B), run
 *       to run.  Workgroups are assigned per sample (per-workgroup partials, then a fixed-order total, as ofd_nan_mse_sum), for any
 *       B >= 1 -- more samples than workgroups included -- and any n_per_sample >= 1.  Loads and stores are 16 bytes wide when
 *       n_per_sample % 4 == 0 and the pointers are 16-byte aligned, scalar otherwise.
 *   R4. ofd_nan_mse_rows_grad: dpred[b, i] = 0 where either side is NaN, otherwise
 *       (float)(2.0 * gout[0] * weight[b] / result[1]) * (p - t): the backward of result[0] / result[1].  A result whose [1] is 1.0 gives
 *       the gradient of the plain weighted sum result[0].  gout is a device scalar; only result[1] is read.
 * Argument errors (a NULL pred / target / result / gout / dpred, B < 1, n_per_sample == 0) return before any GPU work. */
size_t ofd_nan_mse_rows_result_doubles(int B);
int ofd_nan_mse_rows(const float* pred, const float* target, const float* weight, int B, size_t n_per_sample, double* result,
                     void* stream);
int ofd_nan_mse_rows_grad(const float* pred, const float* target, const float* weight, int B, size_t n_per_sample,
                          const double* result, const float* gout, float* dpred, void* stream);

/* ---------------------------------------------------------------- optimiser (FD:131-134) ---
 * torch.optim.Adam(lr, weight_decay) semantics (L2 in the gradient) preceded by
 * clip_grad_norm_(max_norm) (exp_base.py:192,205), multi-tensor, no host synchronisation.
 * table: device array of {float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
 * uint64 numel}; tasks: device arrays (tensor index, chunk index) with ofd_adam_chunk() elements
 * per chunk.  sqnorm_acc (n_tasks + 1 doubles: [0] the squared norm, then one partial sum per task, added in a
 * fixed order -- the same gradients give the same clip coefficient bit for bit), clip_coef (1 float) and optional
 * total_norm are device scratch/outputs.  step counts from 1.  max_norm <= 0 disables clipping.  The clip coefficient is
 * min(1, max_norm / (norm + 1e-6)) with a NaN kept (a NaN norm makes every element NaN, as clip_grad_norm_ does) and 0 for an
 * infinite norm.  The bias corrections 1 - beta^step are formed in double from the float betas and rounded once.  Rows may be
 * 4-byte aligned only. */
int ofd_adam_chunk(void);
int ofd_adam_step(const void* table, const unsigned* task_tensor, const unsigned* task_chunk, int n_tasks,
                  double* sqnorm_acc, float* clip_coef, float* total_norm, float max_norm, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* ofd_adam_step plus an exponential moving average (EMA) of the parameters, kept inside the same three launches: the step kernel
 * has each new parameter value in a register and spends one more read and one more write per element on its average, instead
 * of a second pass over every parameter.  Rows carry one more pointer: {float* param; const float* grad; float* exp_avg;
 * float* exp_avg_sq; uint64 numel; float* ema}; every other argument is ofd_adam_step's, and param / exp_avg / exp_avg_sq come out
 * bit for bit as from ofd_adam_step.  Per element, after p_new is stored: ema = ema_d * ema + ema_omd * p_new, the two products each
 * rounded to fp32 and then added (no fused multiply-add).  ema_d = 0, ema_omd = 1 therefore leaves ema an exact copy of the new
 * parameters.  The caller rounds ema_omd = 1 - d itself (optim.ema_decay_at), the kernel never forms 1 - ema_d. */
int ofd_adam_step_ema(const void* table, const unsigned* task_tensor, const unsigned* task_chunk, int n_tasks,
                      double* sqnorm_acc, float* clip_coef, float* total_norm, float max_norm, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, float ema_d, float ema_omd,
                      void* stream);

/* ------------------------------------------------------------------------ UNet (DD:272-417) -
 * Handle-based executor of the whole forward: one call runs every kernel of the network on
 * `stream`.  Parameters keep the reference's state-dict names. */
typedef struct ofd_unet ofd_unet;

typedef struct {
    int dim;            /* 64 (must be a multiple of 64) */
    int channels;       /* UNet input channels = x channels + cond channels (1..48: 5 / 6 / 9 pixel space, 3 / 19 autoencoder, 18 / 33 / 35 latent) */
    int out_dim;        /* 1..16 (2 for the diffusion UNet) */
    int eps_mode;       /* 0: eps 1e-5 everywhere (reference precision 32);
                           1: per-site eps the reference uses under bf16 autocast (DD:107,122) */
    int no_time;        /* 0: Unet(time_in=True) (the diffusion UNet).  1: Unet(time_in=False) (DD:306-324, FD:110 with
                           is_diffusion=False; flow_learner.py:93-98): no time MLP, ResnetBlocks without scale/shift
                           (DD:192-195), the `t` argument of the forward calls is ignored and may be NULL */
    int n_levels;       /* resolution levels: 0 or 4 = dim_mults (1,2,4,8) (the diffusion UNet; 0 keeps configs written before this
                           field existed meaning 4), 3 = dim_mults (1,2,4) (the reference's Autoencoder, flow_pred.py:17-35; requires
                           no_time = 1; trains like the four-level UNet).  channels 1..48, out_dim 1..16. */
} ofd_unet_config;

int ofd_unet_create(const ofd_unet_config* cfg, ofd_unet** out);
void ofd_unet_destroy(ofd_unet* u);
/* number of parameter tensors, and name / element count of the i-th (reference state-dict order) */
int ofd_unet_num_params(const ofd_unet* u);
const char* ofd_unet_param_name(const ofd_unet* u, int i);
size_t ofd_unet_param_numel(const ofd_unet* u, int i);
int ofd_unet_param_shape(const ofd_unet* u, int i, int* dims4);   /* returns ndim (1..4) */
/* copy fp32 parameter i from a device buffer (reference layout, e.g. OIHW) into the engine */
int ofd_unet_set_param(ofd_unet* u, int i, const float* dev_src, size_t numel, void* stream);
/* weight standardisation + bf16 re-layout of everything set so far; call after set_param */
/* Zero-copy alternative to ofd_unet_set_param: the executor reads its parameters from the caller's flat fp32
 * device buffer (parameter i at floats [ofd_unet_param_offset(i), +numel), ofd_unet_param_floats in all; 16-byte
 * aligned, must outlive the handle or the next bind).  Call ofd_unet_prepare again whenever its contents change. */
int ofd_unet_bind_param_buffer(ofd_unet* u, float* dev_params, size_t floats);
int ofd_unet_prepare(ofd_unet* u, void* stream);
size_t ofd_unet_workspace_bytes(const ofd_unet* u, int B, int H, int W);
/* x: (B,Cx,H,W) fp32, cond: (B,Cc,H,W) fp32 or NULL (Cx+Cc == channels), t: (B,) int64,
 * out: (B,out_dim,H,W) fp32.  H and W must be multiples of 8.
 * Memory of `out` (and of every device pointer of this header): ordinary device memory of the GPU the stream belongs to, as
 * hipMalloc / torch's caching allocator return it (coarse-grained).  When H*W is a multiple of 128 the final 1x1 conv (DD:361) is
 * computed on the tile of final_res_block's res_conv and reaches `out` as hardware fp32 atomic adds onto a buffer the call zeroes first
 * (two addends per element, order-free); fine-grained / host-coherent / managed allocations, where such atomics are not guaranteed, are
 * not supported for `out` -- ofd_unet_set_debug_taps(u, 1) selects the unfused final conv (plain stores) for such a buffer. */
int ofd_unet_forward(ofd_unet* u, const float* x, int Cx, const float* cond, int Cc, const int64_t* t,
                     float* out, int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* debug: copy a named intermediate of the LAST forward (e.g. "init_conv", "downs.0.0",
 * "mid_attn") as NCHW fp32 into dst (numel checked).  Returns OFD_ERR_ARG for unknown names. */
/* hipGraph replay of ofd_unet_forward (launch-bound regimes: small images, the 1000-step sampling loop).  When enabled,
 * the inputs are copied to fixed staging buffers inside the workspace, the first call of a (workspace, shape, stream)
 * configuration runs eagerly, the second is captured into a graph and every later one is a single hipGraphLaunch.
 * Bit-identical results.  Ignored while profiling is on (per-kernel events need individual launches). */
int ofd_unet_set_graph(ofd_unet* u, int enabled);
/* Two half-batch forwards on two streams (even B >= 2; ignored while profiling or graph replay is on).  enabled: 1 on, 0 off, -1 (the
 * handle's default) on for batches of at least 2^21 pixels in all -- at the BASELINE size the step is 1.3 % faster, small problems are
 * launch-bound and keep one stream.  Samples are independent
 * in every kernel of the network (GroupNorm, LinearAttention and attention are per sample: DD:172-268), so samples [0, B/2) run on
 * `stream` and samples [B/2, B) run the same launch sequence on a second, library-owned stream that starts `offset_blocks` blocks
 * (ResnetBlock / attention block granularity; < 0 keeps the current value) behind the first: the HBM-bound kernels of one half share
 * the chip with the MFMA-bound kernels of the other.  `stream` waits for both halves before the call's successors run.  Results are
 * bit-identical to the one-stream forward per sample.  ofd_unet_workspace_bytes already covers the two half contexts. */
int ofd_unet_set_split_streams(ofd_unet* u, int enabled, int offset_blocks);
int ofd_unet_read_tap(ofd_unet* u, const char* name, float* dst, size_t numel, void* stream);
/* debug: materialise EVERY named intermediate of the inference forward.  Off (default), final_res_block's 64-channel output is not:
 * the final 1x1 conv (DD:361) then rides on the tile of its producer (out_dim 2, H*W a multiple of 128) and "final_res_block" is
 * not a tap.  The two forms sum the 64 products of a pixel in different orders (equal to fp32 rounding). */
int ofd_unet_set_debug_taps(ofd_unet* u, int enabled);
/* elementwise glue of the reference's Autoencoder (flow_pred.py:38-58) folded into the forward, inference and training (the backward
 * differentiates the clamps as torch.clamp does: gradient where -1 <= v <= 1, v recomputed by the final conv's backward kernel):
 *   x_affine / cond_affine = 1: the input staging feeds 2 v - 1 instead of v for the x / cond planes (encoder 2x-1; decoder cat(l, 2x-1));
 *   out_mode 0: plain output; 1: clamp(clamp(v, -1, 1) / out_div, -1, 1) (encode, and FD:145-148 with out_div = latent_max);
 *   2: (clamp(v, -1, 1) + 1) / 2 (decode).  Applied by the final 1x1 conv's kernel on its fp32 result (out_mode != 0 runs the unfused
 *   final conv).  Changing it drops captured graphs. */
int ofd_unet_set_glue(ofd_unet* u, int x_affine, int cond_affine, int out_mode, float out_div);
/* deterministic backward (default: the environment variable OFD_DETERMINISTIC, else off).  The backward accumulates parameter
 * gradients from many workgroups with float atomics, whose order -- and so the last bits of the sums -- changes from run to run
 * (torch's cuDNN weight gradients behave the same way in the reference).  Enabled, every such accumulation goes through a 64-bit
 * fixed-point shadow (csrc/det.h: value * 2^38, integer atomics, order-independent) that is flushed into the fp32 gradient
 * before anyone reads it: two backward passes over the same tape give bit-identical gradients.  Costs 8 bytes per parameter and
 * accumulator of extra memory and a few small launches per layer.  ofd_unet_deterministic_misses: accumulations (since creation)
 * that found no shadow and fell back to float atomics (0 for the UNet of this library; -1 on error). */
int ofd_unet_set_deterministic(ofd_unet* u, int enabled);
long ofd_unet_deterministic_misses(ofd_unet* u);
/* per-kernel-class device time of forwards run with profiling enabled (HIP events on the
 * stream the kernels are launched on).  classes: see ofd_unet_prof_name(). */
int ofd_unet_set_profiling(ofd_unet* u, int enabled);
int ofd_unet_prof_count(const ofd_unet* u);
const char* ofd_unet_prof_name(const ofd_unet* u, int i);
/* resolves the recorded events (host-synchronises) -> ms, launches and flops/bytes summed since last reset */
int ofd_unet_prof_read(ofd_unet* u, int i, double* ms, long long* launches, double* flops, double* bytes);
int ofd_unet_prof_reset(ofd_unet* u);
/* optional: append one CSV row per launch (class,label,ms,flops,bytes) to `path` whenever the
 * events are resolved; NULL/"" disables */
int ofd_unet_prof_dump_path(ofd_unet* u, const char* path);

/* ---------------------------------------------------------------- single ops (parity tests) -
 * NHWC bf16 activations (uint16_t* = raw bf16 bits).  These are the kernels the executor
 * launches, exposed one by one so that each can be checked against the oracle. */
typedef struct {
    const void* src;        /* bf16 NHWC */
    int channels;           /* channels taken from this source (multiple of 64; 7x7: 16) */
    int src_channels;       /* channel count (pixel stride) of the source tensor */
    int ch_offset;          /* first channel taken */
    int upsample;           /* 1: source is (H/2,W/2), read with nearest x2 (DD:91) */
    int unshuffle;          /* 1: source is (2H,2W); this entry is sub-pixel (p1,p2) of DD:97 */
    int p1, p2;
} ofd_conv_src;

typedef struct {
    int B, H, W;            /* OUTPUT spatial size */
    int ksize;              /* 1, 3 or 7; 2 = one phase of an up-sampled 3x3 (see up2_phase) */
    int n_src;              /* 1..4 */
    ofd_conv_src src[4];
    int Cout;               /* multiple of 64 */
    const void* weight;     /* bf16, engine layout (ofd_conv_weight_layout) */
    const float* bias;      /* fp32 [Cout] or NULL */
    const float* in_scale;  /* optional prologue: y = silu(x*in_scale[b][c] + in_shift[b][c]) */
    const float* in_shift;  /* fp32 [B][Cin] */
    const void* residual;   /* optional epilogue add: bf16 NHWC (B,H,W,Cout) */
    const void* res_act;    /* optional epilogue add of silu(r*res_scale[b][c] + res_shift[b][c]) */
    const float* res_scale;
    const float* res_shift;
    void* out;              /* bf16 NHWC (B,H,W,Cout) */
    float* gn_partial;      /* optional: GroupNorm partial sums [b][8 groups][8x32 tile][4 wave slots][Cout/64][2] (sum, sum
                               of squares of the stored values; group-major so that ofd_gn_finalize reads one contiguous
                               run per (sample, group)), ofd_conv_gn_partial_count floats */
    void* out2;             /* split output (data gradients of a conv over two concatenated sources): channels */
    const void* residual2;  /*   [0, split) -> out / residual with pixel stride split, [split, Cout) -> out2 / residual2 */
    int split;              /*   with stride Cout - split; multiple of 64, 0 = off */
    int up2_phase;          /* ksize 2 only: 1 + py*2 + px.  Upsample(x2, nearest) + 3x3 (DD:89-93) as four 2x2 convs on
                               the LOW-RES source: B,H,W are the low-res size, `out` is the (2H, 2W) tensor and this
                               launch writes its pixels (2y+py, 2x+px); weights from ofd_conv_upsample_phase_weight_prep
                               (+ (up2_phase-1) * 4*Cin*Cout elements).  5 = all four phases in one launch (`weight` =
                               the base of the four kernels): the phases of a pixel tile run together on one XCD */
} ofd_conv_args;

int ofd_conv_forward(const ofd_conv_args* a, void* stream);
/* the same 3x3 convolution with every 2x2 block of output pixels SUMMED in the epilogue: `out` (and `residual`, added there) is the
 * (H/2, W/2) tensor.  This is the data gradient of Upsample(x2, nearest) + conv (DD:89-93) taken straight into the low-resolution
 * source's gradient: a = the data-gradient configuration above (source dY at (H, W), tap-flipped transposed weights).  H, W even,
 * Cout a multiple of 64 and not the 64 -> 64 case, no split output / GroupNorm statistics / activation residual. */
int ofd_conv_forward_pool2(const ofd_conv_args* a, void* stream);
size_t ofd_conv_gn_partial_count(int B, int H, int W, int Cout);   /* floats */
/* OIHW fp32 -> engine bf16 layout [tap][Cin/8][Cout][8]; eps < 0: plain conv, else weight
 * standardisation with that eps (DD:109-112).  cin_pad: Cin rounded up (7x7: 16).
 * unshuffle != 0: Cin index is c*4+p1*2+p2 (DD:97) and is regrouped as (p1,p2) major. */
size_t ofd_conv_weight_elems(int Cout, int Cin_pad, int ksize);
int ofd_conv_weight_prep(const float* w_oihw, void* w_out, int Cout, int Cin, int Cin_pad, int ksize,
                         float ws_eps, int unshuffle, void* stream);

/* ---------------------------------------------------------------- conv backward (training) --
 * (conv_wgrad.hip: ofd_conv_wgrad, ofd_conv7_wgrad, ofd_conv7_wgrad_c, their _bias forms, ofd_channel_sum; conv_bwd.hip: the layout kernels around them)
 * data gradient  : run ofd_conv_forward on dY (source, Cout channels) with the weights produced by
 *                  ofd_conv_dgrad_weight_prep (tap-flipped, in/out transposed); output has Cin channels;
 *                  ofd_grad_scatter applies the adjoint of concat / up-sample (mode 1) / unshuffle (mode 2).
 * weight gradient: ofd_conv_wgrad accumulates dW[tap][Cin][Cout] (fp32, zeroed by the caller) from the
 *                  forward's input sources and dY; ofd_conv_wgrad_finish converts to the OIHW parameter
 *                  gradient, through weight standardisation when ws_eps >= 0 (DD:109-112).
 * bias gradient  : ofd_channel_sum (out[C] += column sums; zero it first). */
/* 3x3 OIHW fp32 -> the four collapsed 2x2 kernels of the phase decomposition, 4 x [4 taps][Cin/8][Cout][8] bf16 */
int ofd_conv_upsample_phase_weight_prep(const float* w_oihw, void* w_out, int Cout, int Cin, void* stream);
int ofd_conv_dgrad_weight_prep(const void* w_fwd, void* w_t, int Cout, int Cin, int ksize, void* stream);
int ofd_conv_wgrad(const ofd_conv_args* fwd, const void* dy, float* dw_acc, void* stream);
int ofd_conv7_wgrad(const void* x16, const void* dy, float* dw_acc, int B, int H, int W, void* stream);
/* the same for an input packed to `channels` = 8, 16, 32 or 48 (pixel stride); dw_acc is [49][channels][64] */
int ofd_conv7_wgrad_c(const void* x, const void* dy, float* dw_acc, int B, int H, int W, int channels, void* stream);
/* ofd_conv_wgrad / ofd_conv7_wgrad_c as the training executor calls them: the same launch also ADDS the column sums of dY (the bias
 * gradient) to dbias [Cout] fp32 (64 for the 7x7 conv); dbias must not be NULL.  With dbias a 1x1 conv of Cout = 384 over one plain source
 * runs the 64 x 64 block kernel, not the to_qkv kernel (which sums no bias). */
int ofd_conv_wgrad_bias(const ofd_conv_args* fwd, const void* dy, float* dw_acc, float* dbias, void* stream);
int ofd_conv7_wgrad_bias(const void* x, const void* dy, float* dw_acc, float* dbias, int B, int H, int W, int channels, void* stream);
/* data gradient of the 7x7 init conv w.r.t. its first cx <= 16 input channels: dy NHWC bf16 [B][H][W][64], w_t the tap-flipped transposed
 * weights of ofd_conv_dgrad_weight_prep (Cin = cin_pad = 16, 32 or 48) -> dx NCHW fp32 [B][cx][H][W] = scale * conv_transpose(dy)
 * (written, not added; deterministic: a gather, no atomics) */
int ofd_conv7_dgrad(const void* dy, const void* w_t, int cin_pad, float* dx, int cx, int B, int H, int W, float scale, void* stream);
int ofd_conv_wgrad_finish(const float* dw_acc, const float* w_oihw, float* dst_oihw, int Cout, int Cin, int Cin_pad,
                          int ksize, float ws_eps, int unshuffle, int accumulate, void* stream);
int ofd_grad_scatter(const void* D, int Ctot, int ch_off, void* dst, int C, int B, int H, int W, int mode,
                     int p1, int p2, int accumulate, void* stream);
int ofd_channel_sum(const void* dy, float* out, size_t npix, int C, void* stream);

/* --------------------------------------------------- Block / norm backward (training) --------
 * ofd_gn_silu_backward: backward of out = SiLU(GroupNorm(h) * (scale+1) + shift) (DD:181-187) given
 *   g = dL/dout.  (a, s) is the folded per-(sample, channel) affine of the forward, stats = [B][8][{mean,
 *   rstd}].  Writes dh; ADDS into dgamma / dbeta (fp32 [C]); writes the scale|shift gradient rows into dss
 *   (same indexing as ss; NULL when the block has no time-embedding input).  dconv_bias (may be NULL):
 *   ADDS sum_pixels dh, the bias gradient of the convolution that produced h.  workspace:
 *   ofd_gn_bwd_workspace_floats floats.
 * ofd_layernorm_c_backward: DD:116-125; dx written (or added when accumulate != 0), dg ADDED.
 * ofd_final_conv_backward: DD:361; dx written, dw / db ADDED. */
size_t ofd_gn_bwd_workspace_floats(int B, int H, int W, int C);
int ofd_gn_silu_backward(const void* g, const void* h, const float* a, const float* s, const float* stats,
                         const float* gamma, const float* beta, const float* ss, int ss_stride, int ss_offset,
                         void* dh, float* dgamma, float* dbeta, float* dss, float* dconv_bias, float* workspace,
                         int B, int H, int W, int C, void* stream);
int ofd_affine_silu(const void* h, const float* a, const float* s, void* out, int B, int H, int W, int C, void* stream);
int ofd_layernorm_c_backward(const void* x, const float* g, const void* dy, void* dx, float* dg, size_t npix, int C,
                             float eps, int accumulate, void* stream);
/* the same with `extra` [npix][C] bf16 (may be NULL: then exactly ofd_layernorm_c_backward) added to dx in fp32 before the one rounding:
 * the gradient of a residual branch around the LayerNorm (PreNorm inside Residual: extra = dy of the block).  C = 64, 128, 256, 512. */
int ofd_layernorm_c_backward_residual(const void* x, const float* g, const void* dy, const void* extra, void* dx, float* dg, size_t npix,
                                      int C, float eps, int accumulate, void* stream);
/* DD:361 forward: x NHWC bf16 (C channels) -> out NCHW fp32 (out_dim <= 16), with the glue epilogue of ofd_unet_set_glue (out_mode, out_div) */
int ofd_final_conv(const void* x, const float* w, const float* b, float* out, int B, int H, int W, int C, int out_dim, int out_mode,
                   float out_div, void* stream);
int ofd_final_conv_backward(const void* x, const float* w, const float* dy, void* dx, float* dw, float* db,
                            int B, int H, int W, int C, int out_dim, void* stream);
/* the same through the forward's output glue (ofd_final_conv's out_mode / out_div): dy is dL/d(glue output); the clamps are
 * differentiated as torch.clamp (gradient where -1 <= v <= 1, inclusive), v recomputed from x, w and b with the forward's arithmetic.
 * out_dim <= 4 (C = 64 or 128) or <= 16 (C = 64). */
int ofd_final_conv_backward_glue(const void* x, const float* w, const float* b, const float* dy, void* dx, float* dw, float* db,
                                 int B, int H, int W, int C, int out_dim, int out_mode, float out_div, void* stream);

/* --------------------------------------------------- attention cores, forward + backward -------
 * qkv / dqkv: [B][n][384] bf16 (q | k | v, 4 heads x 32); out / dout: [B][n][128] bf16.
 * LinearAttention core (DD:229-242): forward keeps ctx [B*4][32][32] and ml [B*4][64] (max and 1/sum of
 *   the softmax over pixels) for the backward.  workspace: ofd_la_workspace_floats / ofd_la_bwd_workspace_floats.
 * Softmax attention (DD:256-268): forward keeps lse [B*4][n]; backward needs delta scratch [B*4][n]. */
size_t ofd_la_workspace_floats(int B, int n);
size_t ofd_la_bwd_workspace_floats(int B, int n);
int ofd_linear_attention_core(const void* qkv, void* out, float* ctx, float* ml, float* workspace, int B, int n, void* stream);
int ofd_linear_attention_core_backward(const void* qkv, const void* dout, const float* ctx, const float* ml, void* dqkv,
                                       float* workspace, int B, int n, void* stream);
/* --------------------------------------------------- fused LinearAttention block, one call at a time ------
 * The executor's own launches of a Residual(PreNorm(LinearAttention)) block (DD:81-87, DD:127-135, DD:216-244), exported so that one
 * block can be run and checked alone.  x / y / xn / o2 / dy / dx: [B][n][C] bf16 (pixel-major), C = 64 or 128 as stated per call
 * (ofd_la_weight_prep and ofd_linear_attention_block: also 256 and 512; at 512 the block uses the first 128 channels of each row of y
 * as its own intermediate before it writes the row, so y must not alias x).
 * Any n >= 1 is legal in every call below (rows are whole 16-byte units for every C; pixels past the end of a partial 32-pixel tile
 * are read from a clamped row and masked).  Pointers named x, y and every weight pointer must be 16-byte aligned.
 *
 * Weights in fragment layout (bf16), made by ofd_la_weight_prep from the fp32 parameters wqkv [384][C] (q | k | v rows), g [C] and
 * wout [C][128]:
 *     wq    [C/8][128][8]   128*C elements   = Wq  . diag(g)     (g == NULL: the plain rows -- what the training form takes)
 *     wkv   [C/8][256][8]   256*C elements   = Wkv . diag(g)
 *     woutp [8][2][C][8]    128*C elements   (wout == NULL / woutp == NULL: not written)
 *   No kernel reads past those counts: the buffers need no slack.
 * Scratch: partial = ofd_la_workspace_floats(B, n) floats; ctxfrag = B * 4096 bf16 (8 KB per sample: the combined context of the four
 *   heads as MFMA operand fragments).  Kept for the backward: ctx [B*4][32][32] and ml [B*4][64] fp32, as ofd_linear_attention_core.
 *
 * ofd_linear_attention_block (C = 64, 128): inference form; y = x + LayerNorm_g2(to_out.0(attention(LayerNorm_g(x)))); wq / wkv carry g.
 *   Three launches, no atomics: the same inputs give the same bits.
 * ofd_linear_attention_block_train (C = 64): the training forward; wq / wkv are the PLAIN weights (g == NULL), g_pre is applied to the
 *   LayerNorm output.  Also writes the tape: xn [B][n][64], channels 128..383 (k | v) of qkv [B][n][384] -- channels 0..127 are NOT
 *   written --, o2 [B][n][64] (to_out.0's output), ctx, ml.
 * ofd_linear_attention_core_proj (C = 128, the training forward at that width): ofd_linear_attention_core with the to_out.0 1x1 conv
 *   on the head-output tile: o2 [B][n][C] = wo . out + bo; wo from ofd_conv_weight_prep(Cout = C, Cin = 128, ksize 1): [16][C][8];
 *   bo fp32 [C] or NULL; out may be NULL (the head outputs are then not written).
 * ofd_linear_attention_block_backward (C = 64): the core backward with to_out.0 and to_qkv folded in.  do2 [B][n][64] is the gradient
 *   of the to_out.0 OUTPUT; qkv is read in channels 128..383 only (q is recomputed from xn); dxn [B][n][64] is written;
 *   dw_acc [64][384], dwo_acc [128][64] and dbo [64] (fp32) are ADDED to -- zero them first; ofd_conv_wgrad_finish turns the two
 *   accumulators into OIHW gradients.  Weights (bf16): wq_fwd = ofd_conv_weight_prep(to_qkv: Cout 384, Cin 64, ksize 1) [8][384][8],
 *   wqkv_t = ofd_conv_dgrad_weight_prep of it [48][64][8], wo_fwd = ofd_conv_weight_prep(to_out.0: Cout 64, Cin 128) [16][64][8],
 *   wo_t = ofd_conv_dgrad_weight_prep of it [8][128][8].  workspace: ofd_la_bwd_workspace_floats(B, n) floats. */
int ofd_la_weight_prep(const float* wqkv, const float* g, const float* wout, void* wq, void* wkv, void* woutp, int C, void* stream);
int ofd_linear_attention_block(const void* x, const void* wq, const void* wkv, const void* woutp, const float* bias, const float* g2,
                               float* partial, void* ctxfrag, void* y, int B, int n, int C, float eps_pre, float eps_post, void* stream);
int ofd_linear_attention_block_train(const void* x, const void* wq, const void* wkv, const void* woutp, const float* bias,
                                     const float* g_pre, const float* g2, float* partial, void* ctxfrag, float* ctx, float* ml,
                                     void* xn, void* qkv, void* o2, void* y, int B, int n, int C, float eps_pre, float eps_post,
                                     void* stream);
int ofd_linear_attention_core_proj(const void* qkv, void* out, float* ctx, float* ml, float* workspace, const void* wo,
                                   const float* bo, void* o2, int C, int B, int n, void* stream);
int ofd_linear_attention_block_backward(const void* qkv, const void* do2, const float* ctx, const float* ml, float* workspace,
                                        const void* xn, const void* wqkv_t, float* dw_acc, void* dxn, const void* wo_fwd,
                                        const void* wo_t, float* dwo_acc, float* dbo, const void* wq_fwd, int C, int B, int n,
                                        void* stream);
int ofd_flash_attention(const void* qkv, void* out, float* lse, int B, int n, void* stream);
int ofd_flash_attention_backward(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                 float* delta, int B, int n, void* stream);

/* --------------------------------------------------- UNet training step -----------------------
 * What autograd does for the reference's training_step (flow_diffuser.py:218-235 ->
 * denoising_diffusion.py:823-891 -> Unet.forward DD:363-417), as two calls:
 *   ofd_unet_train_forward: the forward with every intermediate kept in `workspace`
 *       (ofd_unet_train_workspace_bytes; the workspace must stay untouched until the backward);
 *   ofd_unet_backward: dout = dL/d(out) [B][out_dim][H][W] fp32 -> gradients of all parameters, written
 *       (not accumulated) into the flat fp32 buffer bound with ofd_unet_bind_grad_buffer.  Parameter i
 *       lives at floats [ofd_unet_param_offset(i), +numel) of that buffer (ofd_unet_param_floats in all).
 *       on_ready (may be NULL) is called on the host, in backward order, with each [begin, end) float
 *       range of the buffer as soon as the launches that produce it are enqueued on `stream` -- the
 *       hook for overlapping the data-parallel all-reduce with the rest of the backward. */
typedef void (*ofd_grad_ready_fn)(size_t begin, size_t end, void* user);
size_t ofd_unet_train_workspace_bytes(ofd_unet* u, int B, int H, int W);
size_t ofd_unet_param_floats(const ofd_unet* u);
size_t ofd_unet_param_offset(const ofd_unet* u, int i);
int ofd_unet_bind_grad_buffer(ofd_unet* u, float* dev_grads, size_t floats);
int ofd_unet_train_forward(ofd_unet* u, const float* x, int Cx, const float* cond, int Cc, const int64_t* t,
                           float* out, int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
int ofd_unet_backward(ofd_unet* u, const float* dout, ofd_grad_ready_fn on_ready, void* user, void* stream);
/* ofd_unet_backward plus dL/dx of the first Cdx (<= 16) input channels, written to dx [B][Cdx][H][W] fp32: the data gradient of the 7x7
 * init conv (times 2 when the x glue of ofd_unet_set_glue stages 2 x - 1) */
int ofd_unet_backward_dx(ofd_unet* u, const float* dout, float* dx, int Cdx, ofd_grad_ready_fn on_ready, void* user, void* stream);

/* --------------------------------------------------- forward building blocks of the UNet executor ----
 * ofd_layernorm_c (DD:116-125): out = LN_channels(x) * g (+ residual), NHWC bf16, npix rows of C channels.
 * ofd_time_mlp (DD:139-151, 319-324): sinusoidal embedding -> Linear -> GELU -> Linear; also SiLU(temb).
 * ofd_gn_finalize (DD:181-185): per-(tile, wave, 8-channel) partial sums of a conv epilogue
 *   (ofd_conv_gn_partial_count floats) -> the folded GroupNorm affine (a, s) per (sample, channel), and
 *   optionally the statistics [B][8][{mean, rstd}] the backward needs. */
int ofd_layernorm_c(const void* x, const float* g, const void* residual, void* out, size_t npix, int C, float eps, void* stream);
int ofd_time_mlp(const int64_t* t, const float* w1, const float* b1, const float* w2, const float* b2,
                 float* temb, float* temb_silu, int B, int dim, void* stream);
int ofd_gn_finalize(const float* partial, int B, int H, int W, int C, const float* gamma, const float* beta,
                    const float* ss, int ss_stride, int ss_offset, float* a_out, float* s_out, float* stats_out, void* stream);

/* --------------------------------------------------- the small kernels between them, one launch each (single-op tests) ----
 * The executor's own launchers behind argument checks; nothing here is a different kernel.
 * ofd_block_mlp (DD:193-196, 205-208): ss[b][offsets[i] + j] = weights[i][j][:] . temb_silu[b][:] + biases[i][j] for j < n_out[i], every
 *   ResnetBlock's Linear in ONE launch (grid.y = n_desc).  weights / biases / n_out / offsets are HOST arrays of n_desc entries (device
 *   pointers in the first two; weights[i] is [n_out[i]][tdim], 16-byte aligned when tdim % 4 == 0); the call uploads them as the kernel's
 *   descriptor rows and waits for the stream before it returns.  temb_silu [B][tdim], ss [B][ss_stride]; tdim <= 1024; columns of ss
 *   outside every [offsets[i], offsets[i] + n_out[i]) are not written.
 * ofd_block_mlp_backward: one ResnetBlock's Linear.  dss [B][ss_stride] (columns [offset, offset + n_out) are read), weight [n_out][tdim];
 *   dweight [n_out][tdim], dbias [n_out] and dts [B][tdim] are ADDED to (dts by float atomics: every block adds into it).
 * ofd_time_mlp_backward: t, temb [B][4 dim] as ofd_time_mlp took / wrote them, dts [B][4 dim] = dL/d SiLU(temb); dw1 [4 dim][dim],
 *   db1 [4 dim], dw2 [4 dim][4 dim], db2 [4 dim] are ADDED to; scratch: ofd_time_mlp_backward_scratch_floats(B, dim) floats.  dim <= 256.
 * ofd_resblock_out (DD:214, identity res_conv): out = SiLU(h * a[b][c] + s[b][c]) + x, NHWC bf16, a / s [B][C] fp32, C % 8 == 0.
 * ofd_grad_add: dst = src (accumulate == 0) or dst + src in fp32, rounded once; bf16, elems % 8 == 0.
 * ofd_pack_input (DD:368): cat(x [B][Cx][H][W], cond [B][Cc][H][W]) fp32 -> NHWC bf16 padded with zeros to cpad = 8, 16, 32 or 48
 *   channels; ax / ac != 0: the x / cond planes enter as 2 v - 1.  cond may be NULL when Cc == 0. */
int ofd_block_mlp(const float* temb_silu, const float* const* weights, const float* const* biases, const int* n_out, const int* offsets,
                  int n_desc, float* ss, int B, int tdim, int ss_stride, void* stream);
int ofd_block_mlp_backward(const float* dss, const float* temb_silu, const float* weight, int n_out, int offset, float* dweight,
                           float* dbias, float* dts, int B, int tdim, int ss_stride, void* stream);
size_t ofd_time_mlp_backward_scratch_floats(int B, int dim);
int ofd_time_mlp_backward(const int64_t* t, const float* temb, const float* dts, const float* w1, const float* b1, const float* w2,
                          float* dw1, float* db1, float* dw2, float* db2, float* scratch, int B, int dim, void* stream);
int ofd_resblock_out(const void* h, const float* a, const float* s, const void* x, void* out, int B, int H, int W, int C, void* stream);
int ofd_grad_add(void* dst, const void* src, size_t elems, int accumulate, void* stream);
int ofd_pack_input(const float* x, int Cx, const float* cond, int Cc, void* out, int B, int H, int W, int cpad, int ax, int ac,
                   void* stream);

/* Batched training augmentation in one pass (replaces the per-sample torchvision pipeline of augmentation.py:6-76 behind
 * FlowDiffuser.preprocess(aug=True), flow_diffuser.py:137-138).  img / tgt (B,3,H,W), flow (B,2,H,W) fp32 NCHW; params (B,16) fp32:
 * 0 jitter on, 1 brightness, 2 contrast, 3 saturation, 4 grayscale on, 5 blur on, 6 sigma, 7 h-flip, 8 v-flip, 9 crop on,
 * 10 oy, 11 ox, 12 ch, 13 cw (crop window origin / size as fractions of the image; 1, 1 without a crop).  means_ws: B*2 x 8 bytes of device scratch.
 * reference_semantics == 0 (default of the plugin): geometrically consistent flow -- a flip negates the component along the flipped
 * axis, a crop divides each component by its axis' window fraction.  != 0: the reference's own arithmetic on the flow channels --
 * flips negate the other channel (augmentation.py:37-45), the crop multiplies channel 0 by ch and channel 1 by cw (augmentation.py:47-48).
 * img and tgt must be finite.  flow may hold NaN (the holes of sparse ground truth): a flip moves a NaN with its pixel, a crop makes
 * every output NaN whose bilinear cell holds one (a NaN corner of weight 0 included), and no image output depends on the flow. */
int ofd_augment(const float* img, const float* tgt, const float* flow, const float* params, void* means_ws, float* out_img,
                float* out_tgt, float* out_flow, int B, int H, int W, int reference_semantics, void* stream);
/* the (B, 16) table above from (B, 14) uniform draws in [0, 1) (the caller's RNG: torch's device generator in the plugin), one launch:
 * columns 0, 4, 5, 7, 8, 9 are the decisions u < p (p = 0.4, 0.1, 0.2, 0.3, 0.3, 0.15: augmentation.py:8-35 of the reference), 1-3 = 1 +- 0.1,
 * 6 = max(u / 2, 0.05), the crop window from RandomResizedCrop's scale (0.8, 1.0) and log-uniform ratio (0.9, 1.1). */
int ofd_augment_table(const float* uniforms, float* params, int B, void* stream);

/* the four statistics FlowDiffuser.training_step logs for cond and for flow (flow_diffuser.py:218-235: torch.min, torch.max, torch.mean,
 * torch.mean(torch.std(x, dim=0))) of x (B, n_per_sample) fp32 in one pass: out4 = {min, max, mean, mean over elements of the unbiased standard
 * deviation across the batch} (device); ws: ofd_batch_stats_ws_doubles() doubles of device scratch (partial sums, added in a fixed order).
 * As in torch, one NaN in x makes min, max and mean NaN, and the deviation is NaN for B == 1. */
size_t ofd_batch_stats_ws_doubles(void);
int ofd_batch_stats(const float* x, int B, size_t n_per_sample, double* ws, float* out4, void* stream);

/* FlowCompleter (algorithms/diffusion_animation/diffusion_animation.py:127-246): sparse-flow sampling, its loss and the null-embedding
 * gradient, with no host sync and no float atomics (every output is the same bits for the same inputs).
 *
 * ofd_sparse_flow_sample: dense (B,2,H,W) fp32, u (B,H*W) uniforms in [0,1), k (B,) int32 picks per frame (clamped to [1,8]), null_emb (2,)
 * device.  m = sqrtf(fx*fx + fy*fy), s = batch mean of m (fixed-order sum), w = m + s (1 everywhere when s = 0); frame b keeps the k_b
 * largest keys logf(u) / w, equal keys to the lower index (Efraimidis-Spirakis weighted sampling without replacement).  Writes sparse
 * (B,2,H,W) = null_emb[c] except dense at the picks, picks (B,8) int32 flat indices padded with -1, amax (B,) = max of m per frame.
 * ws: ofd_sparse_flow_ws_bytes(B, H, W) bytes of device scratch, 8-byte aligned.  Four launches. */
size_t ofd_sparse_flow_ws_bytes(int B, int H, int W);
int ofd_sparse_flow_sample(const float* dense, const float* u, const int* k, const float* null_emb, float* sparse, int* picks, float* amax,
                           int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* loss = mean over (b,h,w) of (lmbd + m / amax_b) * ||out - dense||_2 over the two channels (lmbd where amax_b = 0), out / dense (B,2,H,W);
 * result: ofd_completer_loss_result_doubles() doubles of device scratch, [0] the fixed-order sum; loss: one device float */
size_t ofd_completer_loss_result_doubles(void);
int ofd_completer_loss(const float* out, const float* dense, const float* amax, float lmbd, int B, int H, int W, double* result, float* loss,
                       void* stream);
/* dout = gout[0] * (lmbd + m / amax_b) * (out - dense) / ||out - dense|| / (B*H*W), 0 where the norm is 0 */
int ofd_completer_loss_grad(const float* out, const float* dense, const float* amax, const float* gout, float lmbd, int B, int H, int W,
                            float* dout, void* stream);
/* dnull[c] = sum of dx[b,c,h,w] over the pixels that are not picks of their frame (fixed order); ws: ofd_null_grad_ws_doubles() doubles */
size_t ofd_null_grad_ws_doubles(void);
int ofd_null_embedding_grad(const float* dx, const int* picks, int B, int H, int W, double* ws, float* dnull, void* stream);
/* out = sparse with every NaN of channel c replaced by null_emb[c] (FlowCompleter.complete) */
int ofd_sparse_flow_fill(const float* sparse, const float* null_emb, float* out, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OFD_H */

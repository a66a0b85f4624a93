// paths.h — host interfaces between the kernel families' files, and the route of a descriptor.
//
// Every host function that one .hip file defines and another calls is declared here, and both files include
// this header: a changed signature fails to compile instead of linking against the old one.
//
// unet_conv and unet_conv_wgrad choose a kernel family once per call: conv_route (conv.hip) and wgrad_route
// (wgrad.hip) classify the descriptor, and the launch and every query entry point (stats rows, workspace,
// variant name, act_out) read that one answer.  A new kernel form is added in its classifier alone.
#pragma once
#include "common.h"

namespace unet {

// ---- shared descriptor helpers -------------------------------------------------------------------
inline const char* dtype_name(int dtype) { return dtype == UNET_BF16 ? "bf16" : dtype == UNET_F16 ? "fp16" : "fp32"; }

inline int validate_src(const unet_src& s) {
  if (s.kind < 0 || s.kind > UNET_SRC_UP_PLAIN || !s.data || s.C <= 0) return 0;
  if ((s.kind == UNET_SRC_ACT || s.kind == UNET_SRC_POOL_ACT || s.kind == UNET_SRC_UP_ACT) && (!s.scale || !s.shift))
    return 0;
  if (s.gate_p && !s.gate_ab) return 0;
  return 1;
}

// ---- conv5.hip / conv5w.hip: the LDS-DMA 3x3 forms ------------------------------------------------
enum Conv5Form { C5_NONE = 0, C5_WIDE, C5_PLAIN, C5_SPLITK };
struct Conv5Route {
  Conv5Form form = C5_NONE;   // C5_WIDE: conv5w (128 output channels per workgroup); C5_SPLITK needs d->workspace
  int mi = 0;                 // wave-tile rows of the form
  int splitk = 1;             // split count of the shape (> 1 also where a null d->workspace keeps form C5_NONE)
  size_t workspace = 0;       // bytes of the shape's split-K slabs, whatever d->workspace holds
  int stats_rows = 0;         // partial rows the form writes (forward stats or bnb sums)
  bool act_out_ok = false;    // the form can write src[0]'s transformed input to d->act_out
};
Conv5Route conv5_route(const unet_conv_desc* d);   // 16-bit descriptors (reads the UNET_CONV5* switches once)
int conv5_run(const unet_conv_desc* d, const Conv5Route& r, hipStream_t st);
bool conv5w_ok(const unet_conv_desc* d, int* mi);   // conv5w.hip: *mi = its wave-tile rows (8 or 4)
int conv5w_stats_rows(const unet_conv_desc* d, int mi);
int conv5w_run(const unet_conv_desc* d, int mi, int prio, hipStream_t st);

// ---- the other conv families ---------------------------------------------------------------------
bool smallcin_conv_ok(const unet_conv_desc* d);     // smallcin.hip
int smallcin_stats_rows(const unet_conv_desc* d);
bool smallcin_is_mfma(const unet_conv_desc* d);
int smallcin_conv(const unet_conv_desc* d, hipStream_t st);
bool pw_conv_ok(const unet_conv_desc* d);           // pw.hip
int pw_conv_rows(const unet_conv_desc* d);
int pw_conv(const unet_conv_desc* d, hipStream_t st);
int pw_conv_variant(const unet_conv_desc* d, char* buf, int len);
int conv_generic(const unet_conv_desc* d, hipStream_t st);   // conv_generic.hip
int pack_tiles_launch(int dtype, int count, const unet_pack_job* jobs, hipStream_t st);   // pack.hip

// the template tuple of a conv3 / conv2 kernel: WM x WN waves, NTN 16-channel tiles and MI rows per wave, RAW
// loads per halo item.  The y epilogue of a conv3 tile with ntn == 1 and raw == 1 also reduces the
// BatchNorm-backward sums.
struct ConvTile {
  int wm, wn, ntn, mi, raw;
};

enum ConvPath { CONV_SMALLCIN, CONV_PW, CONV_GENERIC, CONV_CONV5W, CONV_CONV5, CONV_CONV5_SPLITK, CONV_CONV3, CONV_CONV2 };
struct ConvRoute {
  ConvPath path;
  ConvTile tile;          // CONV_CONV3 / CONV_CONV2
  Conv5Route c5;          // mi, split count, workspace and act_out of the conv5 forms (16-bit pipelined descriptors)
  int stats_rows;         // rows the call writes: forward stats, or bnb sums (of the separate reduction if that follows)
  bool bnb_in_epilogue;   // the conv reduces the bnb_* sums itself; else unet_bn_bwd_reduce follows it
};
ConvRoute conv_route(const unet_conv_desc* d);   // conv.hip

// ---- weight gradients ----------------------------------------------------------------------------
enum WgradPath { WGRAD_SMALLCIN, WGRAD_PW, WGRAD_WGRAD5, WGRAD_WGRAD2, WGRAD_WGRAD };
struct WgradRoute {
  WgradPath path;
  size_t workspace;   // bytes unet_conv_wgrad needs in d->workspace
  char variant[64];
};
WgradRoute wgrad_route(const unet_wgrad_desc* d);   // wgrad.hip

bool smallcin_wgrad_ok(const unet_wgrad_desc* d);   // smallcin.hip
size_t smallcin_wgrad_ws(const unet_wgrad_desc* d);
bool smallcin_wgrad_is_mfma(const unet_wgrad_desc* d);
int smallcin_wgrad(const unet_wgrad_desc* d, hipStream_t st);
bool pw_wgrad_ok(const unet_wgrad_desc* d);         // pw.hip
size_t pw_wgrad_ws(const unet_wgrad_desc* d);
int pw_wgrad(const unet_wgrad_desc* d, hipStream_t st);
bool wgrad5_eligible(const unet_wgrad_desc* d, size_t* ws_bytes);   // wgrad5.hip
int wgrad5_run(const unet_wgrad_desc* d, hipStream_t st);
bool wgrad2_eligible(const unet_wgrad_desc* d, size_t* ws_bytes);   // wgrad2.hip
int wgrad2_run(const unet_wgrad_desc* d, hipStream_t st);

// dw (+)= the fixed-order sum of `splits` slabs of `total` floats
int wgrad_reduce2_launch(const float* ws, int splits, long long total, float* dw, int accum, hipStream_t st);   // wgrad2.hip
// the same through PW_RG partial slabs in `scratch` (many splits of a small weight tensor)
int slab_reduce_two_pass(const float* ws, int splits, long long total, float* scratch, float* dw, int accum,
                         hipStream_t st);   // pw.hip

}  // namespace unet

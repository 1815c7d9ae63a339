// loss_eval_optim.hip: the translation unit of the losses, the evaluation meters, the optimizers, the inference merges and image ingest.
// It holds no kernel and no namespace of its own: the library-wide pieces (the error string, the version, the ABI stamp) are at its end,
// and every subject is a self-contained header (own includes, own namespace; kernels, argument checks and entry points together)
// compiled as part of this unit, in this order:
//   loss_rows.h      workgroup geometry (cvk_ce_blocks), chunk staging and weighted pixel terms of the losses; k_lv_clear
//   edt.h            exact Euclidean distance transform of label maps
//   boundary_f1.h    boundary F1 contour map and counts
//   surface_dist.h   Hausdorff, HD95 and ASSD (uses edt.h and boundary_f1.h)
//   boundary_iou.h   Boundary IoU and trimap counts on a chessboard depth map (uses boundary_f1.h)
//   eval_meters.h    class histogram, arg-max, confusion counts
//   optim_flat.h     AdamW, momentum SGD, the per-iteration log row
//   grad_flat.h      global-norm clipping and gradient accumulation
//   crop_aug.h       crop training: class-balanced window selection, resize + crop + pad + blur + LUT + flip
//   components.h     connected components of a class map (union-find over tiles) and the removal of small regions
//   crf.h            local-window mean-field CRF refinement of a prediction (a register-blocked stencil over an LDS tile)
//   loss_ce.h        softmax cross-entropy, plain and with class weights, label smoothing and a reduction
//   loss_ohem.h      OHEM cross-entropy with its radix select of the k-th largest pixel loss
//   loss_lovasz.h    Lovász-softmax with its segmented radix sort
//   loss_boundary.h  boundary loss over the signed distance maps of edt.h
//   loss_seg.h       fused focal + soft-Dice loss
//   loss_kd.h        knowledge-distillation loss (cross-entropy + temperature KL)
//   calibration.h    calibration meter (ECE tables, NLL, Brier) and the Newton temperature fit
//   infer_merge.h    the inference merges: test-time augmentation views and sliding windows
//   ingest.h         uint8 frames to normalised NHWC; the fused train / val transform
// A new subject gets a header of that kind, not lines here.
#include "cvk_common.h"
#include "loss_rows.h"
#include "edt.h"
#include "boundary_f1.h"
#include "surface_dist.h"
#include "boundary_iou.h"
#include "eval_meters.h"
#include "optim_flat.h"
#include "grad_flat.h"
#include "crop_aug.h"
#include "components.h"
#include "crf.h"
#include "loss_ce.h"
#include "loss_ohem.h"
#include "loss_lovasz.h"
#include "loss_boundary.h"
#include "loss_seg.h"
#include "loss_kd.h"
#include "calibration.h"
#include "infer_merge.h"
#include "ingest.h"

// ---- library-wide pieces ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void cvk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int cvk_version(void) { return CVK_VERSION; }
#ifndef CVK_ABI_HASH
#error "CVK_ABI_HASH is not defined: build through csrc/Makefile (it hashes include/cvk.h)"
#endif
extern "C" uint64_t cvk_abi_hash(void) { return CVK_ABI_HASH; }
extern "C" const char* cvk_last_error_string(void) { return g_err; }

// What every unit of the library shares: the public header, the list of the library's switches, the two normalisation constants.
// Device primitives: dg_device.h; a subsystem's argument blocks and launchers: dg_corr_args.h, dg_head_args.h, dg_eval_args.h, dg_loss_args.h, dg_data_args.h, dg_aux_args.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/depthg_corr.h"

// Switches of the library - the complete list (tests/test_host_cpu.py fails on a getenv or a tested macro not named here).
// Test seams, read in every build; each selects a second route that must give the same bits (tests/test_gpu_configs.py):
//   DG_FOLD_INTRA=0   the intra pair-set's streamed-side gradient by k_gs instead of k_corr2's fold (dg_api_corr.hip make_plan)
//   DG_SPLIT_MASKS=0  the dense grid's exact-mask chain in sequence on the caller's stream, no side stream (dg_api_corr.hip)
//   DG_C2_WALK=dynamic|static   the walk of k_corr2's persistent workgroups (dg_corr2.hip)
// Measurement instruments, compiled only into a `make EXTRA=-DDG_DEVTOOLS` build (results unchanged, timing perturbed; the capture
// every launcher uses for them - variable, device buffer, file - and the kernels' stamp macro: dg_devtools.h):
//   DG_STAMPS=<file>, DG_BLOCKLOG=<file>   phase stamps / per-block timeline of the fused kernel (with -DDG_STAMP_BUILD for
//                                           k_corr_main, -DC2_STAMPS [-DC2_STAMP_N=n -DC2_BLOCKSTAMPS_ONLY] or -DC2_BLOCKLOG for k_corr2)
//   DG_HEAD_STAMPS=<file>, DG_DH_STAMPS=<file>   phase stamps of k_head_fwd / k_head_dh, k_head_dh2
//   DG_SMALL_DEBUG=1  block 0 of k_corr_small prints its phase stamps
// Python side: DG_POISON=1 (depthg_amd/ops.py: poisoned buffers, tests/test_gpu_poison.py), DEPTHG_LIB=<path> (another build).
// Tuning constants (#ifndef X / #define X value, no other code behind them): C2_PF, PF, GS_CW, GS_NB, DG_STAGGER, DG_PRIO,
// DG_F_IG, DENSE_TPB, COMB_HB, COMB_HB_HM, HEAD_FWD_PD, HEAD_SPLIT_TARGET.

#define DG_EPS_NORM 1e-10f          // F.normalize eps, reference src/modules.py:790
#define DG_EPS_NORM_DEFAULT 1e-12f  // F.normalize's default eps (src/modules.py:664-669 call it without one): dg_probe.hip, dg_eval.hip, dg_crf.hip

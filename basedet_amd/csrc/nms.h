// What rcnn_ops.hip's RPN proposal chain needs of nms.hip: the candidate layout of an image's pyramid levels, the workspace sizes of the
// joint and the per-level NMS, and their two run functions (launches on `st`, no launch check: the caller's BD_CHECK_LAUNCH covers them).
#pragma once
#include "common.h"

constexpr int NMS_MAX = 16384;                  // boxes of one joint problem (the sort's keys: 128 KiB of LDS)
constexpr int NMSL_CAP = 2048;                  // candidates per (image, level): pre_k <= TOPK_MAX

// level l of an image: pixels from pix_off[l], candidates cand_off[l] .. cand_off[l + 1] of the image's C
struct RpnLevels { int pix_off[BD_MAX_SEGS]; int cand_off[BD_MAX_SEGS + 1]; int L; };

size_t bd_nms_joint_ws_bytes(int B, int C);
size_t bd_nms_levels_ws_bytes(int N, int L, int C, int post_k);

// B problems of capacity C; items with score == -inf are absent.  keep[b * keep_ld ..], num_keep[b]; max_output <= 0: no limit.
int bd_nms_joint_run(const float* boxes, const float* scores, const int32_t* idxs, int B, int C, float thr, int max_output, int keep_ld,
                     int32_t* keep, int32_t* num_keep, unsigned char* ws, hipStream_t st);
// N images of C candidates with the level as class id, level by level + merge: the joint form's keep[n * post_k ..] bit for bit
int bd_nms_levels_run(const float* boxes, const float* scores, const RpnLevels& lv, int N, int C, float thr, int post_k, int32_t* keep,
                      int32_t* num_keep, unsigned char* ws, hipStream_t st);

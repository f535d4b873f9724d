/*
 * segmentation.h -- C ABI of the post-processing of a YOLO instance-segmentation head (libgs_rasterizer_hip.so): ultralytics' Detect /
 * Segment inference decode, ops.non_max_suppression (per class, greedy, on class-offset boxes) and ops.process_mask (crop at proto
 * resolution, bilinear upsampling, logit > 0), ORed into one mask and folded into a frame's motion mask. The network's convolutions stay
 * with the caller. No launch copies anything to the host or waits for the device: the detection count stays in device memory.
 * Device pointers unless marked host; float32 and contiguous. Returns 0 or a negative GSR_ERR_* code (gs_rasterizer.h);
 * gsr_last_error() has the text. stream: hipStream_t or NULL.
 */
#ifndef SEGMENTATION_H_INCLUDED
#define SEGMENTATION_H_INCLUDED

#include <stddef.h>
#include "gs_rasterizer.h"   /* GSR_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_YOLO_MAX_LEVELS 4
#define GSR_YOLO_MAX_ANCHORS 8192   /* 640 x 480 has 6300 anchors, 640 x 640 has 8400 */
#define GSR_YOLO_REG_MAX 16          /* DFL bins per box side */
#define GSR_YOLO_DET_HEAD 7          /* a detection row: x1 y1 x2 y2 score class anchor, then nm mask coefficients */

/* gsr_yolo_workspace_size: bytes of the workspace gsr_yolo_detect needs for `anchors` anchors (the sum of h * w over the levels);
 * 0 when anchors is outside [1, GSR_YOLO_MAX_ANCHORS]. */
size_t gsr_yolo_workspace_size(int anchors);

/* gsr_yolo_detect: the detections of one image. Level l (of `levels`): level_hw[2 l], level_hw[2 l + 1] = its grid (h, w), host;
 * level_stride[l] its stride in pixels, host; head[l] = [64 + nc, h, w] (the 4 x 16 DFL logits, then the nc class logits); coef[l] =
 * [nm, h, w]. Anchors are numbered level by level, row-major. An anchor is a candidate when its largest class sigmoid exceeds conf,
 * and its argmax class (the first of equal maxima) is one of classes[0 .. n_classes) (host). Candidates are ordered by score
 * descending, then anchor ascending; NMS suppresses a candidate whose IoU with a kept box of its class exceeds iou, and each class keeps
 * its first max_det survivors. dets: [max_dets, 7 + nm] rows in that order; counts (3 ints): detections written, candidates, NMS
 * survivors before max_det. workspace: gsr_yolo_workspace_size(anchors) bytes. */
int gsr_yolo_detect(int levels, const int* level_hw, const float* level_stride, const float* const* head, const float* const* coef, int nc,
                    int nm, const int* classes, int n_classes, float conf, float iou, int max_det, void* workspace, float* dets, int max_dets,
                    int* counts, void* stream);

/* gsr_yolo_masks: the union of the instance masks of the first min(counts[0], max_dets) rows of dets (as gsr_yolo_detect writes them),
 * proto [nm, proto_h, proto_w] with height = 4 proto_h and width = 4 proto_w, both multiples of 32. Per detection: logits = coef . proto,
 * zero outside the box scaled by (proto_w / width, proto_h / height) (proto pixel (row r, column c) kept iff x1 <= c < x2 and
 * y1 <= r < y2), bilinear upsampling to height x width (align_corners=False), > 0. yolo_mask [height, width] (bytes 0 / 1) receives the
 * union, when given; motion [height, width] (bool bytes), when given, is cleared where the union is set (motion &= ~yolo). */
int gsr_yolo_masks(int max_dets, const float* dets, const int* counts, int nm, const float* proto, int proto_h, int proto_w, int height, int width,
                   unsigned char* yolo_mask, unsigned char* motion, void* stream);

#ifdef __cplusplus
}
#endif

#endif

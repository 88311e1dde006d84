// Job descriptors and launch constants shared by the kernel sources
// (mirrored by the host-side packing in ops/hip.py and ops/hip_sparse.py).
#pragma once

#define WAVE 64
#define HIST_BLOCK 256

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be a ROCm device tensor")

struct HistJob {
  int start;        // row segment [start, end) in rowbuf
  int end;
  int hist_idx;     // output histogram index
  int fg_start;     // feature group [fg_start, fg_end)
  int fg_end;
  int first_block;  // first grid block assigned to this job
  int num_blocks;
};

struct PartJob {
  int start;
  int end;
  int feature;
  int split_bin;
  int default_left;
  int first_block;
  int num_blocks;
};

struct LeafJob {
  int start;
  int end;
  int parity;
  float value;
  int first_block;
  int num_blocks;
};

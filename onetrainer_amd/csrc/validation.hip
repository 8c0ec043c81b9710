// Validation pass: per-concept (sum, count) of the per-sample losses, kept on the device.
//
// The reference's validation loop (modules/trainer/GenericTrainer.py:319-389) runs batch size 1 and reads
// loss.item() after every image, then averages per concept on the host.  Here the loss kernels' per-sample losses
// (losses_out of csrc/diffusion.hip) of a whole batch are added into acc[concept] on the device, and acc is read
// once after the last batch.
//
// One workgroup, no atomics: concept c belongs to one lane, which walks the batch in ascending b and adds in double.
// The result is therefore a pure function of the sequence of batches, equal bit for bit to a sequential float64
// sum on the host, and two runs give the same bits.
#include "common.h"

// acc: double [n_concepts][2] = (sum, count).  A sample whose index is outside [0, n_concepts) is skipped.
__global__ void __launch_bounds__(256) validation_accumulate_kernel(const float* losses, const int* concept_index,
                                                                    int B, int n_concepts, double* acc) {
  __shared__ float l_s[LOSS_MAX_B];
  __shared__ int c_s[LOSS_MAX_B];
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    l_s[b] = losses[b];
    c_s[b] = concept_index[b];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < n_concepts; c += blockDim.x) {
    double sum = acc[2 * c], cnt = acc[2 * c + 1];
    bool hit = false;
    for (int b = 0; b < B; ++b)
      if (c_s[b] == c) {
        sum += (double)l_s[b];
        cnt += 1.0;
        hit = true;
      }
    if (hit) {
      acc[2 * c] = sum;
      acc[2 * c + 1] = cnt;
    }
  }
}

// losses f32 [B], concept_index i32 [B] (device), acc f64 [n_concepts][2] (device, 8-byte aligned).
// concept_index_host: the same B indices in host memory, or nullptr; when given, an index outside [0, n_concepts)
// is OTAMD_EINVAL before anything is launched (the kernel skips such a sample either way).
OTAMD_API int otamd_validation_accumulate(const float* losses, const int* concept_index,
                                          const int* concept_index_host, int B, int n_concepts, double* acc,
                                          hipStream_t s) {
  if (!losses || !concept_index || !acc || B <= 0 || B > LOSS_MAX_B || n_concepts <= 0) return OTAMD_EINVAL;
  if (((uintptr_t)acc & 7) || ((uintptr_t)losses & 3) || ((uintptr_t)concept_index & 3)) return OTAMD_EINVAL;
  if (concept_index_host)
    for (int b = 0; b < B; ++b)
      if (concept_index_host[b] < 0 || concept_index_host[b] >= n_concepts) return OTAMD_EINVAL;
  validation_accumulate_kernel<<<1, 256, 0, s>>>(losses, concept_index, B, n_concepts, acc);
  OTAMD_CHECK_LAUNCH();
  return OTAMD_OK;
}

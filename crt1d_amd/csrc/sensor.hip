// Sensor-band outputs (include/crt1d_hip_sensor.h): the finish kernel of the level kernels' sensor forms.  With several band slices per
// column each workgroup leaves the partial sums of its slice (sens_row, crt_internal.hpp); this kernel adds them.
#include "crt_internal.hpp"

namespace crt {
namespace {

// One thread per output element (v, r, q, s): the partial sums of the slices that meet the support of sensor band s, added in ascending
// slice order -- the slices a workgroup skipped in sens_row are skipped here, so nothing unwritten is read.
template <bool MASKED>
__device__ __forceinline__ void sens_finish_body(const SensArgs& sn, long long nv, int nslice, int per, int nb, int nsel, ColMask m, int nt) {
  const int nsens = sn.nsens;
  const long long n = nv * nsel * 4 * nsens;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = (int)(i % nsens);
  const int q = (int)((i / nsens) % 4);
  const int r = (int)((i / (4LL * nsens)) % nsel);
  const long long v = i / (4LL * nsens * nsel);
  if constexpr (MASKED)
    if (col_skipped(m, (int)(v / nt))) return;  // (before the slice sums of the column are read)
  double* const o = sn.o[q];
  if (!o) return;
  const int f = sn.first[s], e = f + sn.count[s];
  double z = 0.0;
  bool any = false;
  for (int sl = 0; sl < nslice; ++sl) {
    const int lo_s = sl * per, hi_s = min(lo_s + per, nb);
    if (max(f, lo_s) >= min(e, hi_s)) continue;
    const double p = sn.part[(((v * nslice + sl) * nsel + r) * 4 + q) * nsens + s];
    z = any ? z + p : p;
    any = true;
  }
  o[(v * nsel + r) * nsens + s] = z;
}

// the masked entries (include_mask/crt1d_hip_masked.h): an element of a skipped column (v / nt) keeps its bits, and its slice sums are not
// read.  (In front of k_sens_finish, which stays the last kernel of the unit.)
__global__ __launch_bounds__(256) void k_sens_finish_masked(SensArgs sn, long long nv, int nslice, int per, int nb, int nsel, int nt, ColMask m) {
  sens_finish_body<true>(sn, nv, nslice, per, nb, nsel, m, nt);
}

__global__ __launch_bounds__(256) void k_sens_finish(SensArgs sn, long long nv, int nslice, int per, int nb, int nsel) {
  sens_finish_body<false>(sn, nv, nslice, per, nb, nsel, ColMask{}, 1);
}

}  // namespace

int launch_sens_finish(const SensArgs& sn, long long nv, int nslice, int per, int nb, int nsel, hipStream_t s, ColMask mask, int nt) {
  const long long n = nv * nsel * 4 * sn.nsens;
  const long long nblk = (n + 255) / 256;
  if (nblk > 0x7fffffffLL) return CRT_ERR_UNSUPPORTED;
  if (mask.skip) return launch_kernel(k_sens_finish_masked, dim3((unsigned)nblk), 256, 0, s, sn, nv, nslice, per, nb, nsel, nt, mask);
  return launch_kernel(k_sens_finish, dim3((unsigned)nblk), 256, 0, s, sn, nv, nslice, per, nb, nsel);
}

}  // namespace crt

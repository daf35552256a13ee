// Table of per-instance HBM fields (base pointer + bytes per instance) used by the generic
// instance-copy kernel and by snapshot/restore.
#pragma once
#include <stddef.h>
#include <vector>
struct DrlgxField {
  char *base;
  size_t stride;  // bytes per instance (multiple of 4)
  int cls;        // 0 = belief/simulator state, 1 = virtual-map planes (rebuilt every step), 2 = ground-truth landmarks
  // what of the slice is live: 0 = all of it; 1 / 2 / 3 = unit_bytes per pose / landmark / factor of the SOURCE instance
  // (its counters): the copy moves the live part only, so that a large capacity costs short trajectories nothing
  // (4, in the compact restore table only: unit_bytes per pose of the source's VALID covariance panel - its header's count; jd)
  int unit;
  int unit_bytes;
  int pad;        // > 0: bytes of the slice this entry stands for (a sub-slice: base points at it, stride is the whole slice's); 0: all of it
};

// The bytes of an entry's slice an instance copy moves, `count` being the source's count of the entry's unit (ignored at unit 0):
// per-unit entries end at the count, rounded up to 16 bytes and clamped to the slice.  One formula for every copy kernel and the host.
__host__ __device__ inline size_t drlgx_field_live_bytes(size_t stride, int unit, int unit_bytes, int pad, int count) {
  if (!unit) return pad > 0 ? (size_t)pad : stride;
  const size_t b = ((size_t)(count > 0 ? count : 0) * (size_t)unit_bytes + 15) & ~(size_t)15;
  return b < stride ? b : stride;
}
// ... and the items they are moved as: 16-byte items where the stride keeps every instance's slice 16-byte aligned, 4-byte words otherwise
__host__ __device__ inline bool drlgx_field_by_words(size_t stride) { return (stride & 15) != 0; }
__host__ __device__ inline size_t drlgx_field_items(size_t stride, size_t live) { return drlgx_field_by_words(stride) ? live / 4 : live / 16; }

// ---- the compact restore (k_restore_compact, k_misc.hip) ----
// Its table: what a lazy restore copies - the entries of class 0 and 2 in the order of `fields`, those moved as 16-byte items
// first (then, with panels, the pose marginals jd as an entry of unit 4), those moved as words last.  n16 = how many of the first kind.
constexpr int kRestoreMaxEntries = 32;  // (the kernel's prefix search takes five steps; a longer table is served by the generic kernel)
inline std::vector<DrlgxField> drlgx_restore_table(const std::vector<DrlgxField> &fields, const double *jd, int P_max, int *n16) {
  std::vector<DrlgxField> tab;
  for (const DrlgxField &f : fields)
    if (f.cls != 1 && !drlgx_field_by_words(f.stride)) tab.push_back(f);
  if (jd) tab.push_back(DrlgxField{reinterpret_cast<char *>(const_cast<double *>(jd)), (size_t)P_max * 6 * sizeof(double), 0, 4, 6 * (int)sizeof(double), 0});
  *n16 = (int)tab.size();
  for (const DrlgxField &f : fields)
    if (f.cls != 1 && drlgx_field_by_words(f.stride)) tab.push_back(f);
  return tab;
}

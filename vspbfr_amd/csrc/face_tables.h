// Shared host check of the whole-photo entries (face_warp.hip: crop and paste, plain and anti-aliased; color_fix.hip): one face's
// destination -> source tables against the table buffer, before anything is launched.
#pragma once
#include "vsp_common.h"

namespace vspface {

constexpr int kTableLimit = 1 << 30;
constexpr uint64_t kTwoGiB = 1ull << 31;

// every entry of one face's tables below 2^30 in magnitude (so that cx + ax cannot wrap) and inside the table buffer
// Item: vsp_face_item or vsp_face_aa_item (tab_off, nx, ny)
template <class Item>
int check_tables(const char* what, int i, const Item& it, const int32_t* tables, size_t table_ints) {
  VSP_REQUIRE(it.nx >= 0 && it.ny >= 0 && it.nx <= VSP_FACE_MAX_SIDE && it.ny <= VSP_FACE_MAX_SIDE, "%s: face %d: table extents %d x %d", what,
              i, it.nx, it.ny);
  const uint64_t n = 2ull * (uint64_t)it.nx + 2ull * (uint64_t)it.ny;
  VSP_REQUIRE(it.tab_off >= 0 && (uint64_t)it.tab_off + n <= (uint64_t)table_ints, "%s: face %d: tables outside the %zu table entries", what, i,
              table_ints);
  const int32_t* t = tables + it.tab_off;
  for (uint64_t k = 0; k < n; ++k)
    VSP_REQUIRE(t[k] > -kTableLimit && t[k] < kTableLimit, "%s: face %d: table overflow (entry %llu = %d, magnitude 2^30 or more)", what, i,
                (unsigned long long)k, t[k]);
  return VSP_OK;
}

}  // namespace vspface

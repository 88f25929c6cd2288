// bam_aux_walk.h -- one step through a BAM record's aux block, shared by everything that walks one: set_xf
// (smooth_host.cpp), the XF walk of smooth_walk_kernel (bam_smooth.hip) and both aux_int (bam_reader.h on the host,
// bam_device_internal.h on the device).  Plain C++, no includes but <stdint.h>: tests/aux_walk_harness.cpp builds from this
// header alone and runs it under AddressSanitizer / UndefinedBehaviorSanitizer.
//
// The rule is htslib's skip_aux: a walk GIVES UP -- the block is left as it is, the tag counts as absent -- on a type it
// does not know, on a tag cut off before its type byte, on a B array whose header or whose elements do not fit in the
// block (the count is unsigned: a negative one is a huge one), on a Z / H without its terminator, and on any value that
// ends behind the block.  Nothing is read or skipped past `end`; sizes are compared against `end - p` BEFORE the walk
// advances, in unsigned arithmetic without a product that could wrap.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVDSS_AUX_HD __host__ __device__ __forceinline__
#else
#define SVDSS_AUX_HD inline
#endif

enum { SVDSS_AUX_GIVE_UP = -1 };
enum { SVDSS_AUX_ABSENT = -1, SVDSS_AUX_BAD = -2 };

// [p, end) starts at a tag (two name bytes, a type byte, the value): the bytes of its value, so that the next tag is at
// p + 3 + the result; SVDSS_AUX_GIVE_UP if the walk cannot go on.  A result >= 0 lies inside the block: 3 + result <= end - p.
SVDSS_AUX_HD int64_t svdss_aux_value_size(const uint8_t* p, const uint8_t* end) {
  if (end - p < 3) return SVDSS_AUX_GIVE_UP;
  const uint64_t room = (uint64_t)(end - p) - 3;      // bytes behind the type byte
  const uint8_t* v = p + 3;
  uint64_t sz;
  switch ((char)p[2]) {
    case 'A': case 'c': case 'C': sz = 1; break;
    case 's': case 'S': sz = 2; break;
    case 'i': case 'I': case 'f': sz = 4; break;
    case 'Z': case 'H': {
      uint64_t z = 0;
      while (z < room && v[z]) ++z;
      if (z == room) return SVDSS_AUX_GIVE_UP;        // no terminator
      return (int64_t)(z + 1);
    }
    case 'B': {
      if (room < 5) return SVDSS_AUX_GIVE_UP;
      const char st = (char)v[0];
      const uint64_t cnt = (uint64_t)v[1] | ((uint64_t)v[2] << 8) | ((uint64_t)v[3] << 16) | ((uint64_t)v[4] << 24);
      const uint64_t es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4;
      if (cnt > (room - 5) / es) return SVDSS_AUX_GIVE_UP;
      return (int64_t)(5 + cnt * es);                 // (cnt * es <= room - 5: no wrap)
    }
    default: return SVDSS_AUX_GIVE_UP;
  }
  return sz <= room ? (int64_t)sz : (int64_t)SVDSS_AUX_GIVE_UP;
}

SVDSS_AUX_HD bool svdss_aux_is_int_type(char ty) { return ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I'; }

// bam_aux_update_int's search: the first tag a b of an integer type in [begin, end).  Returns the offset of its value from
// `begin` (the whole value lies inside the block; value_bytes = its size), SVDSS_AUX_ABSENT if the walk reaches the end of
// the block without one, SVDSS_AUX_BAD if it gives up.
SVDSS_AUX_HD int64_t svdss_aux_find_int(const uint8_t* begin, const uint8_t* end, char a, char b, int32_t& value_bytes) {
  value_bytes = 0;
  const uint8_t* p = begin;
  while (p < end) {
    const int64_t sz = svdss_aux_value_size(p, end);
    if (sz < 0) return SVDSS_AUX_BAD;
    if ((char)p[0] == a && (char)p[1] == b && svdss_aux_is_int_type((char)p[2])) {
      value_bytes = (int32_t)sz;
      return (int64_t)(p + 3 - begin);
    }
    p += 3 + sz;
  }
  return SVDSS_AUX_ABSENT;
}

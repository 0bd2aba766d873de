// TEST-ONLY host build of the four k256 products with speculative columns (fe_k256.hpp: mul, sqr, mul_add2, mul_add_sqr without
// ECGPU_K256_BRANCHFREE) on raw 256-bit operands (possibly >= p), with the ECGPU_SPEC_NOTE hook recording per speculative site
// whether its carry flag was raised: tests/test_hosttwin_k256_spec_carry.py.  The portable fallback of the mac_colM_nN_s1 forms
// leaves the carry of the speculative product out of c.hi and returns it, and mac_spec_fix adds it, exactly as the device code does.
// The product headers are compiled into a namespace of this file's own, because the hook changes the inline functions' bodies and the
// other hosttwin translation units compile them without it.
// With -DHOSTTWIN_SPEC_CARRY_MAIN the file is a program of its own that checks the same properties (for a sanitizer build).
#include <stdint.h>
#include <string.h>
#ifdef HOSTTWIN_SPEC_CARRY_MAIN
#include <stdio.h>
#include <vector>
#endif
static uint32_t g_raised, g_seen, g_bad_site;
static const char* g_form;
static void spec_note(const char* site, int column, bool raised) {
  if (strcmp(site, g_form) != 0 || column < 0 || column > 14) g_bad_site++;
  g_seen |= 1u << column;
  if (raised) g_raised |= 1u << column;
}
#define ECGPU_SPEC_NOTE(site, column, raised) spec_note(site, column, raised)
#define ecgpu ecgpu_spec_twin          // only across the product headers below; every system header is included above
#include "fe_k256.hpp"
#undef ecgpu
using namespace ecgpu_spec_twin;

static const char* FORM_NAMES[4] = {"mul", "sqr", "mul_add2", "mul_add_sqr"};

extern "C" {
// op: 0 mul(a, b)   1 sqr(a)   2 mul_add2(a, b, e, f)   3 mul_add_sqr(a, b, e).  Operands and results are n x 8 little-endian words;
// out is the raw, weakly reduced value.  masks[i]: bit K set when the site of column K was raised by input i.  seen[0]: bit K set when
// the hook of column K ran at all.  Returns the number of hook calls whose site name or column was wrong (0), -1 for a bad op.
int ht_k256_spec_carry_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* e, const uint32_t* f, uint32_t* out,
                          uint32_t* masks, uint32_t* seen, int n) {
  if (op < 0 || op > 3) return -1;
  g_form = FORM_NAMES[op];
  g_seen = 0; g_bad_site = 0;
  for (int i = 0; i < n; i++) {
    FeK256 x, y, u, v, r;
    memcpy(x.v, a + 8 * i, 32); memcpy(y.v, b + 8 * i, 32); memcpy(u.v, e + 8 * i, 32); memcpy(v.v, f + 8 * i, 32);
    g_raised = 0;
    switch (op) {
      case 0: k256::mul(r, x, y); break;
      case 1: k256::sqr(r, x); break;
      case 2: k256::mul_add2(r, x, y, u, v); break;
      case 3: k256::mul_add_sqr(r, x, y, u); break;
    }
    memcpy(out + 8 * i, r.v, 32);
    masks[i] = g_raised;
  }
  seen[0] = g_seen;
  return (int)g_bad_site;
}
// the same products through the exact columns (every product with its carry addition): what the speculative ones must equal bit for bit
int ht_k256_exact_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* e, const uint32_t* f, uint32_t* out, int n) {
  if (op < 0 || op > 3) return -1;
  for (int i = 0; i < n; i++) {
    FeK256 x, y, u, v, r;
    memcpy(x.v, a + 8 * i, 32); memcpy(y.v, b + 8 * i, 32); memcpy(u.v, e + 8 * i, 32); memcpy(v.v, f + 8 * i, 32);
    switch (op) {
      case 0: k256::mul_exact(r, x, y); break;
      case 1: k256::sqr_exact(r, x); break;
      case 2: k256::mul_add2_exact(r, x, y, u, v); break;
      case 3: k256::mul_add_sqr_exact(r, x, y, u); break;
    }
    memcpy(out + 8 * i, r.v, 32);
  }
  return 0;
}
}

#ifdef HOSTTWIN_SPEC_CARRY_MAIN
// all-ones operands (they raise sites of every form), near-maximal words and a pseudo-random stream: the speculative products
// equal the exact ones word for word, the all-ones row raises at least one site per form, the random rows none
int main() {
  const int n = 20000;
  std::vector<uint32_t> a(8 * n), b(8 * n), e(8 * n), f(8 * n), o1(8 * n), o2(8 * n), m(n);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); };
  for (int i = 0; i < 8 * n; i++) {
    const int row = i / 8;
    const bool hot = row < 2000;                      // words near 2^32 in the first rows
    uint32_t w[4];
    for (int k = 0; k < 4; k++) { const uint32_t r = next(); w[k] = row == 0 ? 0xFFFFFFFFu : (hot ? (r % 3 == 0 ? r : 0xFFFFFFFFu - (r & 3u)) : r); }
    a[i] = w[0]; b[i] = w[1]; e[i] = w[2]; f[i] = w[3];
  }
  for (int op = 0; op < 4; op++) {
    uint32_t seen = 0;
    if (ht_k256_spec_carry_op(op, a.data(), b.data(), e.data(), f.data(), o1.data(), m.data(), &seen, n) != 0) { printf("op %d: bad hook call\n", op); return 1; }
    if (ht_k256_exact_op(op, a.data(), b.data(), e.data(), f.data(), o2.data(), n) != 0) return 1;
    if (memcmp(o1.data(), o2.data(), 32 * (size_t)n) != 0) { printf("op %d: speculative and exact products differ\n", op); return 1; }
    int raisedrows = 0;
    for (int i = 0; i < n; i++) raisedrows += m[i] != 0;
    for (int i = 2000; i < n; i++) if (m[i] != 0) { printf("op %d: a random row raised a site\n", op); return 1; }
    if (m[0] == 0) { printf("op %d: all ones raised no site\n", op); return 1; }
    printf("%s ok: sites seen 0x%04x, %d of %d rows raised a site\n", FORM_NAMES[op], seen, raisedrows, n);
  }
  return 0;
}
#endif

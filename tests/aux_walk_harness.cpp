// aux_walk_harness.cpp -- csrc/bam_aux_walk.h on the CPU, a program of its own built from that header alone
// (tests/test_aux_walk_host.py builds it with -fsanitize=address,undefined).  Every block is copied into a heap buffer of
// exactly its size, so that a read or a step past `end` is AddressSanitizer's to report; every expected value is written
// out here.  A walk that does not advance never returns: the test's timeout shows it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../svdss_amd/csrc/bam_aux_walk.h"

namespace {
int n_checked = 0, n_failed = 0;

typedef std::string B;   // bytes

B le32(uint32_t v) { B s(4, '\0'); for (int i = 0; i < 4; ++i) s[(size_t)i] = (char)(v >> (8 * i)); return s; }
B tag(const char* name_type, const B& value) { return B(name_type, 3) + value; }
B barr(const char* name, char sub, uint32_t count, size_t payload) { return B(name, 2) + "B" + B(1, sub) + le32(count) + B(payload, '\x07'); }

// an exact-size heap copy (a block of 0 bytes: a 1-byte allocation, walked as [p, p))
struct Block {
  uint8_t* p; size_t n;
  explicit Block(const B& s) : p((uint8_t*)malloc(s.size() ? s.size() : 1)), n(s.size()) { if (n) memcpy(p, s.data(), n); }
  ~Block() { free(p); }
  const uint8_t* end() const { return p + n; }
};

void expect(const char* part, const std::string& what, int64_t got, int64_t want) {
  ++n_checked;
  if (got == want) return;
  ++n_failed;
  printf("%s FAILED: %s: got %lld, want %lld\n", part, what.c_str(), (long long)got, (long long)want);
}

int64_t size_of(const B& s) { Block b(s); return svdss_aux_value_size(b.p, b.end()); }

const int64_t GIVE_UP = -1, ABSENT = -1, BAD = -2;

int part_step() {
  const char* P = "step";
  // every scalar type, exactly fitting and with bytes behind it
  const struct { char ty; int64_t sz; } scalar[] = {{'A', 1}, {'c', 1}, {'C', 1}, {'s', 2}, {'S', 2}, {'i', 4}, {'I', 4}, {'f', 4}};
  for (const auto& t : scalar) {
    const B head = B("ZZ") + B(1, t.ty);
    expect(P, std::string("scalar, exact: ") + t.ty, size_of(head + B((size_t)t.sz, '\x01')), t.sz);
    expect(P, std::string("scalar, more behind: ") + t.ty, size_of(head + B((size_t)t.sz + 5, '\x01')), t.sz);
    // a truncated value: every shorter length, down to none
    for (int64_t k = 0; k < t.sz; ++k) expect(P, std::string("scalar, truncated: ") + t.ty + " " + std::to_string(k), size_of(head + B((size_t)k, '\x01')), GIVE_UP);
  }
  // Z / H with and without terminator
  for (char ty : {'Z', 'H'}) {
    const B head = B("ZZ") + B(1, ty);
    expect(P, std::string("empty string: ") + ty, size_of(head + B(1, '\0')), 1);
    expect(P, std::string("string of 4: ") + ty, size_of(head + "abcd" + B(1, '\0')), 5);
    expect(P, std::string("string of 4, more behind: ") + ty, size_of(head + "abcd" + B(1, '\0') + "NMC" + B(1, '\x02')), 5);
    expect(P, std::string("string without terminator: ") + ty, size_of(head + "abcd"), GIVE_UP);
    expect(P, std::string("string, no byte at all: ") + ty, size_of(head), GIVE_UP);
  }
  // B arrays of every subtype
  const struct { char st; uint32_t es; } sub[] = {{'c', 1}, {'C', 1}, {'s', 2}, {'S', 2}, {'i', 4}, {'I', 4}, {'f', 4}};
  for (const auto& t : sub) {
    const std::string s = std::string("B:") + t.st + " ";
    expect(P, s + "count 0", size_of(barr("ZZ", t.st, 0, 0)), 5);
    expect(P, s + "count 0, more behind", size_of(barr("ZZ", t.st, 0, 9)), 5);
    expect(P, s + "count 1", size_of(barr("ZZ", t.st, 1, t.es)), 5 + (int64_t)t.es);
    expect(P, s + "count 5, exactly fitting", size_of(barr("ZZ", t.st, 5, 5 * t.es)), 5 + 5 * (int64_t)t.es);
    expect(P, s + "count 5, three bytes behind", size_of(barr("ZZ", t.st, 5, 5 * t.es + 3)), 5 + 5 * (int64_t)t.es);
    expect(P, s + "count 5, one byte too long", size_of(barr("ZZ", t.st, 5, 5 * t.es - 1)), GIVE_UP);
    expect(P, s + "count 1, no element", size_of(barr("ZZ", t.st, 1, 0)), GIVE_UP);
    expect(P, s + "count 0x7fffffff", size_of(barr("ZZ", t.st, 0x7fffffffu, 40)), GIVE_UP);
    expect(P, s + "count -1", size_of(barr("ZZ", t.st, 0xffffffffu, 40)), GIVE_UP);
    expect(P, s + "count -2", size_of(barr("ZZ", t.st, 0xfffffffeu, 40)), GIVE_UP);
    expect(P, s + "count INT32_MIN", size_of(barr("ZZ", t.st, 0x80000000u, 40)), GIVE_UP);
    expect(P, s + "count -2, nothing behind", size_of(barr("ZZ", t.st, 0xfffffffeu, 0)), GIVE_UP);
    // the header does not fit: 3 .. 7 bytes of the tag
    const B whole = barr("ZZ", t.st, 0, 0);
    for (size_t k = 3; k < 8; ++k) expect(P, s + "header cut to " + std::to_string(k) + " bytes", size_of(whole.substr(0, k)), GIVE_UP);
  }
  // an unknown type; a block that ends after 0, 1, 2 and 3 bytes of a tag
  expect(P, "unknown type 'Q'", size_of(B("ZZQ") + B(8, '\x01')), GIVE_UP);
  expect(P, "unknown type 0", size_of(B("ZZ") + B(9, '\0')), GIVE_UP);
  expect(P, "no byte", size_of(B()), GIVE_UP);
  expect(P, "1 byte of a tag", size_of(B("X")), GIVE_UP);
  expect(P, "2 bytes of a tag", size_of(B("XF")), GIVE_UP);
  for (char ty : {'A', 'c', 'C', 's', 'S', 'i', 'I', 'f', 'Z', 'H', 'B'}) expect(P, std::string("3 bytes of a tag: ") + ty, size_of(B("XF") + B(1, ty)), GIVE_UP);
  return n_failed;
}

// the walk over a whole block: where the value of the first integer XF is, and how many bytes it has
void find(const char* P, const std::string& what, const B& s, int64_t want_at, int32_t want_n) {
  Block b(s);
  int32_t n = -7;
  const int64_t at = svdss_aux_find_int(b.p, b.end(), 'X', 'F', n);
  expect(P, what + " (offset)", at, want_at);
  expect(P, what + " (bytes)", n, want_n);
}

int part_find() {
  const char* P = "find";
  const B nm = tag("NMi", le32(7)), rg = tag("RGZ", B("grp") + B(1, '\0')), hp = tag("HPC", B(1, '\x02'));   // 7, 7 and 4 bytes
  find(P, "empty block", B(), ABSENT, 0);
  find(P, "no XF", nm + rg + hp, ABSENT, 0);
  const struct { char ty; int32_t sz; } ints[] = {{'c', 1}, {'C', 1}, {'s', 2}, {'S', 2}, {'i', 4}, {'I', 4}};
  for (const auto& t : ints) {
    const B xf = B("XF") + B(1, t.ty) + B((size_t)t.sz, '\x09');
    const std::string s = std::string("XF:") + t.ty + " ";
    find(P, s + "alone", xf, 3, t.sz);
    find(P, s + "first", xf + nm + rg, 3, t.sz);
    find(P, s + "middle", nm + xf + rg, 7 + 3, t.sz);
    find(P, s + "last", nm + rg + hp + xf, 18 + 3, t.sz);
    find(P, s + "after XF:Z", tag("XFZ", B("text") + B(1, '\0')) + xf, 8 + 3, t.sz);
    find(P, s + "after XF:A and XF:f", tag("XFA", "q") + tag("XFf", le32(0x3f800000u)) + xf, 4 + 7 + 3, t.sz);
    find(P, s + "twice: the first", nm + xf + xf, 7 + 3, t.sz);
    // the XF found must have its whole value inside the block
    for (int32_t k = 0; k < t.sz; ++k) find(P, s + "last, value cut to " + std::to_string(k), nm + xf.substr(0, 3 + (size_t)k), BAD, 0);
    // well-formed B arrays of every subtype in front of it, count 0 included
    B arrays;
    for (char st : {'c', 'C', 's', 'S', 'i', 'I', 'f'}) arrays += barr("ZB", st, 0, 0) + barr("ZA", st, 3, 3 * (size_t)((st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4));
    find(P, s + "behind B arrays", arrays + xf, (int64_t)arrays.size() + 3, t.sz);
    // what the walk gives up on in front of it hides it
    find(P, s + "behind an unknown type", tag("ZZQ", "1234") + xf, BAD, 0);
    find(P, s + "behind a B array that overruns", barr("ZZ", 'i', 100, 8) + xf, BAD, 0);
    find(P, s + "behind a B array of count -2", barr("ZZ", 'i', 0xfffffffeu, 0) + xf, BAD, 0);
    find(P, s + "behind a B array of count -1 (bytes)", barr("ZZ", 'c', 0xffffffffu, 0) + xf, BAD, 0);
    find(P, s + "behind a B array of count INT32_MIN (shorts)", barr("ZZ", 's', 0x80000000u, 0) + xf, BAD, 0);
  }
  find(P, "XF:Z alone", tag("XFZ", B("text") + B(1, '\0')), ABSENT, 0);
  find(P, "XF:A, XF:f, XF:H, XF:B", tag("XFA", "q") + tag("XFf", le32(1)) + tag("XFH", B("1A") + B(1, '\0')) + barr("XF", 'C', 2, 2), ABSENT, 0);
  find(P, "1 byte behind the last tag", nm + "X", BAD, 0);
  find(P, "2 bytes behind the last tag", nm + "XF", BAD, 0);
  find(P, "3 bytes behind the last tag", nm + "XFi", BAD, 0);
  find(P, "XF:i then a truncated tag: found first", tag("XFi", le32(5)) + "NMi" + B(1, '\x01'), 3, 4);
  find(P, "unterminated Z last", nm + "RGZgrp", BAD, 0);
  return n_failed;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string part = argc > 1 ? argv[1] : "";
  if (part == "step") part_step();
  else if (part == "find") part_find();
  else { fprintf(stderr, "usage: %s step|find\n", argv[0]); return 2; }
  if (n_failed) { printf("%s: %d of %d checks FAILED\n", part.c_str(), n_failed, n_checked); return 1; }
  printf("%s ok: %d checks\n", part.c_str(), n_checked);
  return 0;
}

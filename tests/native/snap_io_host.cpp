// Host checks of the snapshot blob's cursors (siddhi_amd/csrc/snap_io.h): test infrastructure only.
// Each sih_* check returns 0, or a line number with the reason in msg. tests/snap_io_host.py loads
// them from libsnap_io_host.so; built as a program (main below) the same checks run stand-alone.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../siddhi_amd/csrc/snap_io.h"

namespace {

const size_t SIZES[] = {0, 1, 7, 8, 9};
const size_t HUGE[] = {SIZE_MAX, SIZE_MAX - 1, SIZE_MAX - 6, SIZE_MAX - 7, SIZE_MAX / 2 + 1, SIZE_MAX / 8 + 1};

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      snprintf(msg, cap, "line %d: %s", __LINE__, #cond);               \
      return __LINE__;                                                  \
    }                                                                   \
  } while (0)

// one blob through every Writer call: a word, a range, byte payloads of SIZES (each byte 0xAB), a word
snap::Writer written() {
  snap::Writer w;
  w.put(0x1122334455667788LL);
  const int64_t range[3] = {-1, 0, INT64_MIN};
  w.put(range, range + 3);
  for (size_t n : SIZES) {
    w.put((int64_t)n);
    memset(w.bytes(n), 0xAB, n);
  }
  w.put(-5);
  return w;
}

// the read sequence of that blob; false where a value differs. Throws snap::Error past the end.
bool read_back(snap::Reader& r) {
  bool ok = r.get() == 0x1122334455667788LL;
  const int64_t* range = r.words(3);
  ok = ok && range[0] == -1 && range[1] == 0 && range[2] == INT64_MIN;
  for (size_t n : SIZES) {
    ok = ok && r.get() == (int64_t)n;
    const unsigned char* b = (const unsigned char*)r.bytes(n);
    for (size_t k = 0; k < (n + 7) / 8 * 8; ++k) ok = ok && b[k] == (k < n ? 0xAB : 0);  // (padding stays zero)
  }
  return ok && r.get() == -5;
}

}  // namespace

extern "C" {

int sih_roundtrip(char* msg, size_t cap) {
  const snap::Writer w = written();
  CHECK(w.words().size() == 1 + 3 + 5 + (0 + 1 + 1 + 1 + 2) + 1);
  snap::Reader r(w.words().data(), w.words().size() * 8);
  CHECK(r.left() == w.words().size());
  CHECK(read_back(r));
  CHECK(r.left() == 0);
  snap::Reader ahead(w.words().data(), w.words().size() * 8), copy = ahead;  // a copy scans, the original stays
  copy.skip(4);
  CHECK(ahead.left() == copy.left() + 4 && ahead.get() == 0x1122334455667788LL);
  return 0;
}

// every length in bytes short of the whole blob (so every prefix in words, and lengths that are no
// multiple of 8): the same reads throw "snapshot truncated". Each prefix is a heap block of exactly
// its bytes, so a read past the end is one past the allocation.
int sih_truncated(char* msg, size_t cap) {
  const snap::Writer w = written();
  const size_t total = w.words().size() * 8;
  for (size_t len = 0; len < total; ++len) {
    std::unique_ptr<char[]> blob(new char[len ? len : 1]);
    memcpy(blob.get(), w.words().data(), len);
    snap::Reader r(blob.get(), len);
    CHECK(r.left() == len / 8);
    try {
      (void)read_back(r);
      CHECK(!"a truncated blob read to its end");
    } catch (const snap::Error& ex) {
      CHECK(std::string(ex.what()) == "snapshot truncated");
    }
  }
  return 0;
}

// counts near SIZE_MAX are refused, the cursor stays where it was (no i + n that wraps)
int sih_huge_counts(char* msg, size_t cap) {
  const int64_t four[4] = {1, 2, 3, 4};
  for (size_t n : HUGE)
    for (int call = 0; call < 3; ++call) {
      snap::Reader r(four, sizeof four);
      r.get();
      try {
        if (call == 0) r.bytes(n);
        if (call == 1) r.words(n);
        if (call == 2) r.skip(n);
        CHECK(!"a count near SIZE_MAX was accepted");
      } catch (const snap::Error& ex) {
        CHECK(std::string(ex.what()) == "snapshot truncated");
      }
      CHECK(r.left() == 3 && r.get() == 2);
    }
  return 0;
}

int sih_need(char* msg, size_t cap) {
  snap::need(true, "not thrown");
  try {
    snap::need(false, "snapshot of a different program");
    CHECK(!"need(false) returned");
  } catch (const std::exception& ex) {  // (as the ABI's guard catches it)
    CHECK(std::string(ex.what()) == "snapshot of a different program");
  }
  return 0;
}

}  // extern "C"

int main() {
  char msg[256] = "";
  int bad = 0;
  const struct { const char* name; int (*f)(char*, size_t); } checks[] = {
      {"roundtrip", sih_roundtrip}, {"truncated", sih_truncated}, {"huge_counts", sih_huge_counts}, {"need", sih_need}};
  for (const auto& c : checks) {
    const int rc = c.f(msg, sizeof msg);
    printf("%s: %s\n", c.name, rc ? msg : "ok");
    bad += rc != 0;
  }
  return bad ? 1 : 0;
}

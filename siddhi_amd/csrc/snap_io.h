// snap_io.h -- the snapshot blob's two cursors: a blob is a run of int64 words, byte payloads padded
// with zeros to whole words. No HIP here (tests/native/snap_io_host.cpp builds it for the host).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

// (hidden: a library that includes this exports none of it)
namespace snap __attribute__((visibility("hidden"))) {

// what a blob that cannot be loaded throws (the ABI's guard maps any std::exception to SDH_E_INVALID)
struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void need(bool ok, const char* msg) {
  if (!ok) throw Error(msg);
}

class Writer {
 public:
  void put(int64_t v) { w_.push_back(v); }
  template <class It>
  void put(It first, It last) { w_.insert(w_.end(), first, last); }
  // room for n bytes, zeroed and padded to whole words, for the caller to fill
  void* bytes(size_t n) {
    const size_t o = w_.size();
    w_.resize(o + (n + 7) / 8);
    return w_.data() + o;
  }
  const std::vector<int64_t>& words() const { return w_; }

 private:
  std::vector<int64_t> w_;
};

// A value: a copy reads ahead without moving the original. Every advance goes through words().
class Reader {
 public:
  Reader(const void* blob, size_t len) : p_((const int64_t*)blob), left_(len / 8) {}  // (len in bytes: whole words)
  size_t left() const { return left_; }
  const int64_t* words(size_t n) {
    need(n <= left_, "snapshot truncated");
    const int64_t* p = p_;
    p_ += n;
    left_ -= n;
    return p;
  }
  const void* bytes(size_t n) { return words(n / 8 + (n % 8 != 0)); }
  int64_t get() { return *words(1); }
  void skip(size_t n) { words(n); }

 private:
  const int64_t* p_;
  size_t left_;
};

}  // namespace snap

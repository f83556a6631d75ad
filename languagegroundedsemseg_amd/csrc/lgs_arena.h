// lgs_arena.h -- the bump stack of a coordinate manager's arena block: where in the block an allocation lies.  Host arithmetic only,
// no HIP (tests/cpp/arena_stack_main.cpp runs it on the CPU); lgs_manager.hip owns the device block and the pool fallback.
#pragma once
#include <stddef.h>
#include <vector>

namespace lgs {

class ArenaStack {
 public:
  static size_t rounded(size_t bytes) { return (bytes + 255) / 256 * 256; }
  void reset(size_t capacity) { cap_ = capacity; used_ = peak_ = 0; blks_.clear(); }   // a fresh block (0 bytes: every take fails)
  // the next rounded(bytes) bytes of the block -> true and their offset; false, and nothing changed, where they do not fit
  bool take(size_t bytes, size_t *offset) {
    bytes = rounded(bytes);
    if (bytes > cap_ - used_) return false;
    *offset = used_;
    blks_.push_back({used_, false});
    used_ += bytes;
    if (used_ > peak_) peak_ = used_;
    return true;
  }
  // marks the allocation at `offset` released and pops every released allocation off the top; an unknown offset is ignored
  void release(size_t offset) {
    for (size_t i = blks_.size(); i-- > 0;)
      if (blks_[i].off == offset) { blks_[i].freed = true; break; }
    while (!blks_.empty() && blks_.back().freed) { used_ = blks_.back().off; blks_.pop_back(); }
  }
  size_t capacity() const { return cap_; }
  size_t used() const { return used_; }
  size_t peak() const { return peak_; }   // high-water mark of used()

 private:
  struct Blk { size_t off; bool freed; };
  size_t cap_ = 0, used_ = 0, peak_ = 0;
  std::vector<Blk> blks_;   // allocations not yet popped, in allocation order
};

}  // namespace lgs

// Deferred-reduce queue: the host side of "record now, reduce grouped later", shared by the split-K GEMM reduces
// (gemm.hip, otamd_gemm_defer_*) and the LayerNorm dgamma / dbeta reduces (norm.hip, otamd_layernorm_defer_*).
// A stream in defer mode owns a caller-provided arena (bump-allocated in 256-byte units) and a batch of reduce
// descriptors: a producer takes a slot of arena memory, launches its partial pass into it and pushes a descriptor;
// the batch goes out as one grouped launch when it is full, when the arena is, when the user's clash rule says so,
// and at flush / end.  Host only, no HIP header (tests/csrc/defer_queue_test.cpp builds it with the host compiler):
// the stream key is a template parameter, the grouped launch a callable `int launch(const Batch&, Stream on)` that
// returns 0 or the library's launch-failure code.  Batch is the user's `{int n; unsigned blocks; Desc d[MaxN];}`,
// the struct its grouped kernel takes by value; Desc has `unsigned block0`, its first block in the grouped grid.
// Locking: every method is called with `mu` held.  The users' entry points take it, so it also guards what a user
// keeps per stream beside the queue and lets a user scan the pending batch in place.
#pragma once
#include <stdint.h>

#include <mutex>
#include <type_traits>
#include <unordered_map>

enum { kDeferOk = 0, kDeferInvalid = 1 };   // begin's own codes: the library's OTAMD_OK / OTAMD_EINVAL

template <class Batch, class Stream = void*>
struct DeferQueue {
  using Desc = std::remove_extent_t<decltype(Batch::d)>;
  static constexpr int MaxN = (int)std::extent<decltype(Batch::d)>::value;
  struct State { char* arena = nullptr; long long bytes = 0, used = 0; Batch batch{}; };

  std::mutex mu;
  long long items = 0, launches = 0;   // since load, counted when a batch goes out

  // the stream's state while it is deferring, else nullptr
  State* find(Stream stream) {
    auto it = states_.find(stream);
    return it == states_.end() ? nullptr : &it->second;
  }
  int pending(Stream stream) {
    State* st = find(stream);
    return st ? st->batch.n : 0;
  }
  // enter defer mode (or re-enter with another arena: what the earlier begin left pending goes out first).  arena:
  // 256-byte aligned, >= 1 MiB, kept alive by the caller until end
  template <class Launch>
  int begin(Stream stream, void* arena, long long bytes, Launch&& launch) {
    if (!arena || ((uintptr_t)arena & 255) || bytes < (1 << 20)) return kDeferInvalid;
    State& st = states_[stream];
    const int rc = flush_state(st, stream, launch);
    st.arena = (char*)arena;
    st.bytes = bytes;
    return rc;
  }
  // `need` bytes of arena for the partials of the item about to be pushed; nullptr: the stream is not deferring, or
  // the item can never fit.  The pending batch goes out first when must_flush_first(batch) says so, when it is full,
  // or when the arena is.
  template <class Pred, class Launch>
  void* slot(Stream stream, long long need, Pred&& must_flush_first, Launch&& launch) {
    State* st = find(stream);
    need = (need + 255) / 256 * 256;
    if (!st || need > st->bytes) return nullptr;
    if (must_flush_first(st->batch) || st->batch.n == MaxN || st->used + need > st->bytes)
      flush_state(*st, stream, launch);
    void* p = st->arena + st->used;
    st->used += need;
    return p;
  }
  // record the item whose partials went into the last slot(); nblocks: its share of the grouped grid
  void push(Stream stream, Desc d, unsigned nblocks) {
    Batch& b = find(stream)->batch;
    d.block0 = b.blocks;
    b.blocks += nblocks;
    b.d[b.n++] = d;
  }
  // launch what is pending (stream-ordered) and hand the whole arena back; a no-op off defer mode
  template <class Launch>
  int flush(Stream stream, Launch&& launch) {
    State* st = find(stream);
    return st ? flush_state(*st, stream, launch) : kDeferOk;
  }
  // flush on stream `on` (the caller orders it after `stream`) and leave defer mode
  template <class Launch>
  int end(Stream stream, Stream on, Launch&& launch) {
    State* st = find(stream);
    const int rc = st ? flush_state(*st, on, launch) : kDeferOk;
    states_.erase(stream);
    return rc;
  }

 private:
  template <class Launch>
  int flush_state(State& st, Stream on, Launch&& launch) {
    int rc = kDeferOk;
    if (st.batch.n > 0) {
      rc = launch(st.batch, on);
      ++launches;
    }
    items += st.batch.n;
    st.batch.n = 0;
    st.batch.blocks = 0;
    st.used = 0;
    return rc;
  }

  std::unordered_map<Stream, State> states_;
};

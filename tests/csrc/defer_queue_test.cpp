// Host-only walk through DeferQueue (onetrainer_amd/csrc/defer.h) with a fake grouped launch that records
// (n, blocks, stream, block0 of every descriptor).  Built and run by tests/test_defer_queue_host.py under
// -fsanitize=address,undefined; exits non-zero at the first failed check.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "defer.h"

struct Desc { int tag; unsigned block0; };
constexpr int kMax = 4;
struct Batch { int n; unsigned blocks; Desc d[kMax]; };
using Queue = DeferQueue<Batch, int>;   // streams are plain ints here

struct Launched { int n; unsigned blocks; int stream; std::vector<int> tags; std::vector<unsigned> block0; };
static std::vector<Launched> g_log;
static int g_rc = 0;   // what the fake launch returns

static int fake_launch(const Batch& b, int stream) {
  Launched l{b.n, b.blocks, stream, {}, {}};
  for (int i = 0; i < b.n; ++i) { l.tags.push_back(b.d[i].tag); l.block0.push_back(b.d[i].block0); }
  g_log.push_back(l);
  return g_rc;
}
static bool never(const Batch&) { return false; }

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } \
  } while (0)

constexpr long long MiB = 1 << 20;
alignas(256) static char g_arena[2 * MiB + 256];

// one deferred item: slot, then push (as gemm_impl / ln_param_grads do around their partial pass)
static char* item(Queue& q, int stream, long long need, int tag, unsigned nblocks) {
  char* p = (char*)q.slot(stream, need, never, fake_launch);
  if (p) q.push(stream, Desc{tag, 0}, nblocks);
  return p;
}

int main() {
  Queue q;
  const int S = 7, T = 9;

  // begin: the arena contract
  CHECK(q.begin(S, nullptr, MiB, fake_launch) == kDeferInvalid);
  CHECK(q.begin(S, g_arena + 8, MiB, fake_launch) == kDeferInvalid);
  CHECK(q.begin(S, g_arena, MiB - 1, fake_launch) == kDeferInvalid);
  CHECK(q.find(S) == nullptr && q.pending(S) == 0);
  // off defer mode: no slot, flush and end are no-ops that succeed (end on a stream that never began)
  CHECK(q.slot(S, 256, never, fake_launch) == nullptr);
  CHECK(q.flush(S, fake_launch) == kDeferOk && q.end(S, S, fake_launch) == kDeferOk);
  CHECK(g_log.empty() && q.items == 0 && q.launches == 0);

  CHECK(q.begin(S, g_arena, MiB, fake_launch) == kDeferOk);
  CHECK(q.find(S) && q.find(S)->used == 0 && q.find(S)->bytes == MiB);

  // rollover at MaxN: the bump allocator rounds to 256 bytes, block0 is the prefix sum of the block counts
  for (int i = 0; i < kMax; ++i) {
    CHECK(item(q, S, 100, i, 3 + i) == g_arena + 256 * i);
    CHECK(q.pending(S) == i + 1);
  }
  CHECK(g_log.empty() && q.find(S)->batch.blocks == 3 + 4 + 5 + 6);
  CHECK(item(q, S, 100, 4, 2) == g_arena);   // the full batch went out first and gave the arena back
  CHECK(g_log.size() == 1 && g_log[0].n == kMax && g_log[0].blocks == 18 && g_log[0].stream == S);
  CHECK((g_log[0].block0 == std::vector<unsigned>{0, 3, 7, 12}) && (g_log[0].tags == std::vector<int>{0, 1, 2, 3}));
  CHECK(q.pending(S) == 1 && q.find(S)->batch.d[0].block0 == 0 && q.find(S)->batch.blocks == 2);
  CHECK(q.items == kMax && q.launches == 1);   // counted when the batch goes out, not when pushed

  // flush: launches what is pending; with nothing pending it still hands the arena back
  CHECK(q.flush(S, fake_launch) == kDeferOk);
  CHECK(g_log.size() == 2 && g_log[1].n == 1 && g_log[1].blocks == 2 && q.pending(S) == 0 && q.find(S)->used == 0);
  CHECK(q.slot(S, 512, never, fake_launch) == g_arena && q.find(S)->used == 512);   // a slot never pushed
  CHECK(q.flush(S, fake_launch) == kDeferOk);
  CHECK(g_log.size() == 2 && q.find(S)->used == 0 && q.items == kMax + 1 && q.launches == 2);

  // arena wrap: a flush when used + need > bytes (three 320 KiB items fit 1 MiB, the fourth does not)
  const long long need = 320 * 1024;
  for (int i = 0; i < 3; ++i) CHECK(item(q, S, need, 10 + i, 1) == g_arena + need * i);
  CHECK(g_log.size() == 2 && q.pending(S) == 3);
  CHECK(item(q, S, need, 13, 1) == g_arena);
  CHECK(g_log.size() == 3 && g_log[2].n == 3 && q.pending(S) == 1 && q.find(S)->used == need);
  // exactly the rest of the arena still fits without a flush
  CHECK(item(q, S, MiB - need, 14, 1) == g_arena + need && g_log.size() == 3 && q.find(S)->used == MiB);

  // need larger than the arena (after rounding up to 256): null, nothing launched, nothing more pending
  CHECK(q.slot(S, MiB + 1, never, fake_launch) == nullptr);
  CHECK(q.slot(S, MiB - 255, never, fake_launch) != nullptr);   // rounds to exactly the arena: flushes and fits
  CHECK(g_log.size() == 4 && g_log[3].n == 2 && q.pending(S) == 0);
  CHECK(q.flush(S, fake_launch) == kDeferOk && g_log.size() == 4);
  CHECK(q.slot(S, 2 * MiB, never, fake_launch) == nullptr && q.pending(S) == 0 && q.find(S)->used == 0);

  // the caller's predicate sees the pending batch and forces the flush
  CHECK(item(q, S, 256, 20, 5) && item(q, S, 256, 21, 5) && q.pending(S) == 2);
  int seen = -1;
  auto clash = [&](const Batch& b) { seen = b.n; return b.d[1].tag == 21; };
  CHECK(q.slot(S, 256, clash, fake_launch) == g_arena && seen == 2);
  q.push(S, Desc{22, 0}, 5);
  CHECK(g_log.size() == 5 && g_log[4].n == 2 && g_log[4].blocks == 10 && q.pending(S) == 1);

  // streams are independent
  CHECK(q.begin(T, g_arena + MiB, MiB, fake_launch) == kDeferOk);
  CHECK(item(q, T, 256, 30, 1) == g_arena + MiB && q.pending(T) == 1 && q.pending(S) == 1 && g_log.size() == 5);

  // begin twice: what the first left pending goes out on the stream, the new arena starts empty
  CHECK(q.begin(S, g_arena + 256, MiB + 256, fake_launch) == kDeferOk);
  CHECK(g_log.size() == 6 && g_log[5].n == 1 && g_log[5].stream == S && g_log[5].tags[0] == 22);
  CHECK(q.pending(S) == 0 && q.find(S)->used == 0 && q.find(S)->bytes == MiB + 256);
  CHECK(item(q, S, 256, 23, 1) == g_arena + 256);
  // a rejected begin leaves the running state alone
  CHECK(q.begin(S, nullptr, MiB, fake_launch) == kDeferInvalid && q.pending(S) == 1 && g_log.size() == 6);

  // end with a different launch stream: keyed by S, launched on T; the entry is erased
  const long long items0 = q.items, launches0 = q.launches;
  CHECK(q.end(S, T, fake_launch) == kDeferOk);
  CHECK(g_log.size() == 7 && g_log[6].n == 1 && g_log[6].stream == T && g_log[6].tags[0] == 23);
  CHECK(q.find(S) == nullptr && q.pending(S) == 0 && q.slot(S, 256, never, fake_launch) == nullptr);
  CHECK(q.items == items0 + 1 && q.launches == launches0 + 1);
  CHECK(q.end(S, S, fake_launch) == kDeferOk && g_log.size() == 7);   // already ended: like a stream never begun
  CHECK(q.pending(T) == 1);

  // a failing launch: its code comes back from flush / end / begin, the batch is dropped and counted all the same
  g_rc = 2;
  CHECK(q.flush(T, fake_launch) == 2 && q.pending(T) == 0 && q.find(T)->used == 0);
  CHECK(item(q, T, 256, 31, 1) && q.begin(T, g_arena, MiB, fake_launch) == 2 && q.find(T)->arena == g_arena);
  CHECK(item(q, T, 256, 32, 1) && q.end(T, T, fake_launch) == 2 && q.find(T) == nullptr);
  g_rc = 0;

  // counters: every item that went out, every grouped launch
  long long n = 0;
  for (const Launched& l : g_log) n += l.n;
  CHECK(q.items == n && q.launches == (long long)g_log.size() && n == 17 && g_log.size() == 10);

  // another instance has its own streams and counters
  DeferQueue<Batch, int> other;
  CHECK(other.items == 0 && other.launches == 0 && other.find(T) == nullptr);
  printf("defer_queue_test: ok (%lld items in %zu launches)\n", n, g_log.size());
  return 0;
}

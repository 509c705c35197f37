// The owners of device and pinned memory (rmf_crowdsim_amd/csrc/cs_device_mem.hip.inc) on the host: the generic part of
// the file with a counting, malloc-backed policy that can fail the k-th allocation.  tests/test_device_mem_host.py builds
// this with the address and undefined-behaviour sanitizers and runs it: exit status 0 = every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>

#define CS_DEVICE_MEM_NO_HIP
#include "cs_device_mem.hip.inc"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);   \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

struct Counting {
  static long allocs, frees, syncs, attempts, fail_at;  // fail_at: the attempt (1-based, since arm()) that fails; 0: none
  static std::set<void*> live;
  static void arm(long k) {
    attempts = 0;
    fail_at = k;
  }
  static int allocate(void** p, size_t bytes) {
    *p = nullptr;
    if (++attempts == fail_at) return 2;
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    ++allocs;
    return 0;
  }
  static void release(void* p) {
    CHECK(p != nullptr);             // an owner never frees null
    CHECK(live.erase(p) == 1);       // ... nor anything twice
    std::free(p);
    ++frees;
  }
  static int synchronise(int stream) {
    ++syncs;
    return stream < 0 ? 7 : 0;  // (a negative stream: the wait fails)
  }
};
long Counting::allocs = 0, Counting::frees = 0, Counting::syncs = 0, Counting::attempts = 0, Counting::fail_at = 0;
std::set<void*> Counting::live;

using Bytes = cs_mem::Block<Counting>;
template <class T>
using Buf = cs_mem::Buf<T, Counting>;
using cs_mem::Grow;

void alloc_and_realloc() {
  const long a0 = Counting::allocs, f0 = Counting::frees;
  {
    Buf<uint32_t> b;
    CHECK(b.get() == nullptr && b.bytes() == 0 && b.count() == 0);
    CHECK(b.alloc(10) == 0);
    CHECK(b.get() != nullptr && b.bytes() == 40 && b.count() == 10);
    b.get()[9] = 7u;  // (the sanitizer checks the size)
    CHECK(b.alloc(3) == 0);  // alloc always frees and allocates, smaller or not
    CHECK(b.bytes() == 12 && b.count() == 3);
    CHECK(Counting::allocs == a0 + 2 && Counting::frees == f0 + 1);
    b.release();
    CHECK(b.get() == nullptr && b.bytes() == 0 && Counting::frees == f0 + 2);
    b.release();  // (nothing held: nothing freed)
    CHECK(Counting::frees == f0 + 2);
    CHECK(b.alloc(5) == 0);
  }
  CHECK(Counting::allocs == a0 + 3 && Counting::frees == f0 + 3);  // the destructor freed the last one
}

void reserve_policies() {
  // the growth rules themselves
  CHECK(cs_mem::grown(Grow::exact, 100, 1000) == 100);
  CHECK(cs_mem::grown(Grow::half, 100, 0) == 100 && cs_mem::grown(Grow::half, 101, 100) == 150 &&
        cs_mem::grown(Grow::half, 400, 100) == 400);
  CHECK(cs_mem::grown(Grow::quarter, 100, 0) == 125 && cs_mem::grown(Grow::quarter, 7, 1000) == 8);
  const struct {
    Grow g;
    size_t first, second_need, second;  // bytes held after reserve(100), then after reserve(second_need)
  } cases[] = {{Grow::exact, 100, 101, 101}, {Grow::half, 100, 101, 150}, {Grow::half, 100, 400, 400}, {Grow::quarter, 125, 126, 157}};
  for (const auto& c : cases) {
    Bytes b;
    const long a0 = Counting::allocs, f0 = Counting::frees, s0 = Counting::syncs;
    CHECK(b.reserve(1, 100, c.g) == 0);
    CHECK(b.bytes() == c.first && b.get() != nullptr);
    CHECK(Counting::syncs == s0);  // it held nothing: no wait for the stream
    void* const p = b.get();
    CHECK(b.reserve(1, c.first, c.g) == 0 && b.reserve(1, 1, c.g) == 0 && b.reserve(1, 0, c.g) == 0);  // fits
    CHECK(b.get() == p && b.bytes() == c.first);
    CHECK(Counting::allocs == a0 + 1 && Counting::frees == f0 && Counting::syncs == s0);
    CHECK(b.reserve(1, c.second_need, c.g) == 0);  // does not fit
    CHECK(b.bytes() == c.second);
    CHECK(Counting::allocs == a0 + 2 && Counting::frees == f0 + 1 && Counting::syncs == s0 + 1);  // one wait, for the one free
  }
  {  // the typed form counts in elements
    Buf<double> b;
    CHECK(b.reserve(1, 10, Grow::quarter) == 0 && b.bytes() == 100 && b.count() == 12);
    CHECK(b.reserve(1, 12) == 0 && b.bytes() == 100);
    CHECK(b.reserve(1, 13) == 0 && b.bytes() == 104 && b.count() == 13);
  }
  {  // a failed wait: the error comes back, the scratch is still held, nothing was freed or allocated
    Bytes b;
    CHECK(b.reserve(-1, 64) == 0);  // (nothing held: the stream is not asked)
    void* const p = b.get();
    const long a0 = Counting::allocs, f0 = Counting::frees;
    CHECK(b.reserve(-1, 65) == 7);
    CHECK(b.get() == p && b.bytes() == 64 && Counting::allocs == a0 && Counting::frees == f0);
  }
}

void moves() {
  const long a0 = Counting::allocs, f0 = Counting::frees;
  {
    Buf<int> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(8) == 0);
    int* const pa = a.get();
    Buf<int> c(std::move(a));  // move construction: c holds a's, a holds nothing
    CHECK(c.get() == pa && c.count() == 4 && a.get() == nullptr && a.bytes() == 0);
    CHECK(Counting::frees == f0);
    b = std::move(c);  // move assignment onto a full owner: its own allocation is freed, once
    CHECK(b.get() == pa && b.count() == 4 && c.get() == nullptr && c.bytes() == 0);
    CHECK(Counting::frees == f0 + 1);
    Buf<int>& self = b;
    b = std::move(self);  // (onto itself: nothing happens)
    CHECK(b.get() == pa && Counting::frees == f0 + 1);
    std::swap(a, b);  // what the engine does with its two window lists
    CHECK(a.get() == pa && a.count() == 4 && b.get() == nullptr);
    CHECK(Counting::frees == f0 + 1);
  }
  CHECK(Counting::allocs == a0 + 2 && Counting::frees == f0 + 2);
  static_assert(!std::is_copy_constructible<Bytes>::value && !std::is_copy_assignable<Bytes>::value, "owners do not copy");
  static_assert(!std::is_copy_constructible<Buf<int>>::value && !std::is_copy_assignable<Buf<int>>::value, "owners do not copy");
}

void failures() {
  {  // alloc onto an empty owner
    const long f0 = Counting::frees;
    {
      Buf<int> b;
      Counting::arm(1);
      CHECK(b.alloc(4) == 2);
      CHECK(b.get() == nullptr && b.bytes() == 0);
    }
    CHECK(Counting::frees == f0);  // the destructor freed nothing
  }
  {  // alloc onto a full owner: what it held is freed, once, and it is empty afterwards
    const long f0 = Counting::frees;
    {
      Buf<int> b;
      Counting::arm(2);
      CHECK(b.alloc(4) == 0);
      CHECK(b.alloc(8) == 2);
      CHECK(b.get() == nullptr && b.bytes() == 0 && b.count() == 0);
      CHECK(Counting::frees == f0 + 1);
    }
    CHECK(Counting::frees == f0 + 1);
  }
  for (Grow g : {Grow::exact, Grow::half, Grow::quarter}) {  // reserve, empty and full
    const long f0 = Counting::frees;
    {
      Bytes b;
      Counting::arm(1);
      CHECK(b.reserve(1, 64, g) == 2);
      CHECK(b.get() == nullptr && b.bytes() == 0);
      Counting::arm(2);
      CHECK(b.reserve(1, 64, g) == 0);
      CHECK(b.reserve(1, 1000, g) == 2);
      CHECK(b.get() == nullptr && b.bytes() == 0);
      CHECK(Counting::frees == f0 + 1);
      Counting::arm(0);
      CHECK(b.reserve(1, 8, g) == 0 && b.get() != nullptr);  // (and it serves again)
    }
    CHECK(Counting::frees == f0 + 2);
  }
  Counting::arm(0);
}

void agent_columns() {
  struct F2 {
    float x, y;
  };
  const size_t n = 33;
  const size_t bytes[7] = {n * sizeof(F2),       n * sizeof(F2),       n * sizeof(uint32_t), n * sizeof(uint32_t),
                           n * sizeof(uint32_t), n * sizeof(uint32_t), n * sizeof(uint32_t)};
  for (long k = 1; k <= 7; ++k) {  // the k-th column fails: the k - 1 before it are freed, none is held
    const long a0 = Counting::allocs, f0 = Counting::frees;
    {
      cs_mem::BlockSet<Counting, 7> cols;
      Counting::arm(k);
      CHECK(cols.alloc(bytes) == 2);
      CHECK(Counting::allocs == a0 + (k - 1) && Counting::frees == f0 + (k - 1));
      for (size_t c = 0; c < 7; ++c) CHECK(cols.get(c) == nullptr);
    }
    CHECK(Counting::frees == f0 + (k - 1));
  }
  Counting::arm(0);
  const long a0 = Counting::allocs, f0 = Counting::frees;
  {
    cs_mem::BlockSet<Counting, 7> cols, next;
    CHECK(cols.alloc(bytes) == 0);
    for (size_t c = 0; c < 7; ++c) CHECK(cols.get(c) != nullptr);
    static_cast<uint32_t*>(cols.get(6))[n - 1] = 1u;
    void* const first = cols.get(0);
    CHECK(next.alloc(bytes) == 0);
    cols = std::move(next);  // moves as a whole: the seven old columns are freed, the seven new ones change hands
    CHECK(Counting::frees == f0 + 7 && cols.get(0) != first && next.get(0) == nullptr && next.get(6) == nullptr);
  }
  CHECK(Counting::allocs == a0 + 14 && Counting::frees == f0 + 14);
}

}  // namespace

int main() {
  alloc_and_realloc();
  reserve_policies();
  moves();
  failures();
  agent_columns();
  CHECK(Counting::live.empty());
  CHECK(Counting::frees == Counting::allocs);
  std::printf("%ld allocations, %ld frees, %ld waits, %d checks failed\n", Counting::allocs, Counting::frees, Counting::syncs, g_failed);
  return g_failed ? 1 : 0;
}

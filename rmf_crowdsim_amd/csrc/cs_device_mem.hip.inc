// cs_device_mem.hip.inc — who owns device and pinned memory: the only place that allocates and frees it
// Part of the single translation unit crowdstep_hip.hip (included there, in order).
//
// An owner holds one allocation: a pointer and its size, never out of step (after any failure: null and 0).  It frees in
// its destructor and moves, never copies.  Kernels keep taking raw pointers, from get().
//
// Where the memory comes from is a policy: a struct with the static functions
//   err allocate(void** p, size_t bytes), void release(void* p)   allocate and free; err{} (zero) is success
//   err synchronise(stream)                                       what reserve() waits with before it frees memory that
//                                                                  work queued on `stream` may still use
// Everything above CS_DEVICE_MEM_NO_HIP's guard is plain C++ (tests/cpp/test_device_mem.cpp compiles it with a counting
// policy and no HIP header); the two HIP policies and the aliases the engine uses are below it.

#include <cstddef>
#include <utility>

namespace cs_mem {

// How a kept scratch grows when a need does not fit (it never shrinks).  `held`: the bytes it has.
enum class Grow {
  exact,    // need
  half,     // max(need, 1.5 x held)
  quarter,  // need + need / 4
};
inline size_t grown(Grow g, size_t need, size_t held) {
  if (g == Grow::half) return need > held + held / 2 ? need : held + held / 2;
  if (g == Grow::quarter) return need + need / 4;
  return need;
}

// One allocation, in bytes.
template <class A>
class Block {
 public:
  using err_t = decltype(A::allocate(static_cast<void**>(nullptr), size_t{}));
  Block() = default;
  Block(Block&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Block& operator=(Block&& o) noexcept {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { release(); }

  void* get() const { return p_; }
  size_t bytes() const { return bytes_; }
  void release() {
    if (p_) A::release(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  // frees what it holds, then allocates; empty when that fails
  err_t alloc(size_t bytes) {
    release();
    void* q = nullptr;
    const err_t err = A::allocate(&q, bytes);
    if (err != err_t{}) return err;
    p_ = q;
    bytes_ = q ? bytes : 0;
    return err;
  }
  // Kept scratch: nothing when `need` fits.  Otherwise waits for `stream` if it holds something (and returns that error,
  // still holding it, when the wait fails), frees, and allocates by the policy; empty when the allocation fails.
  template <class Stream>
  err_t reserve(Stream stream, size_t need, Grow g = Grow::exact) {
    if (need <= bytes_) return err_t{};
    if (p_) {
      const err_t err = A::synchronise(stream);
      if (err != err_t{}) return err;
    }
    return alloc(grown(g, need, bytes_));
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// ... and in elements of T.
template <class T, class A>
class Buf {
 public:
  using err_t = typename Block<A>::err_t;
  T* get() const { return static_cast<T*>(b_.get()); }
  size_t bytes() const { return b_.bytes(); }
  size_t count() const { return b_.bytes() / sizeof(T); }
  void release() { b_.release(); }
  err_t alloc(size_t n) { return b_.alloc(n * sizeof(T)); }
  template <class Stream>
  err_t reserve(Stream stream, size_t n, Grow g = Grow::exact) {
    return b_.reserve(stream, n * sizeof(T), g);
  }

 private:
  Block<A> b_;
};

// N allocations that exist together or not at all (the columns of an agent buffer): a failure frees those it already got.
template <class A, size_t N>
class BlockSet {
 public:
  using err_t = typename Block<A>::err_t;
  void* get(size_t k) const { return col_[k].get(); }
  void release() {
    for (Block<A>& c : col_) c.release();
  }
  err_t alloc(const size_t (&bytes)[N]) {
    for (size_t k = 0; k < N; ++k) {
      const err_t err = col_[k].alloc(bytes[k]);
      if (err != err_t{}) {
        release();
        return err;
      }
    }
    return err_t{};
  }

 private:
  Block<A> col_[N];
};

}  // namespace cs_mem

#ifndef CS_DEVICE_MEM_NO_HIP

namespace cs_mem {

struct DeviceAlloc {
  static hipError_t allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
  static hipError_t synchronise(hipStream_t s) { return hipStreamSynchronize(s); }
};
struct PinnedAlloc {
  static hipError_t allocate(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static void release(void* p) { (void)hipHostFree(p); }
  static hipError_t synchronise(hipStream_t s) { return hipStreamSynchronize(s); }
};

}  // namespace cs_mem

using cs_mem::Grow;
using DevBytes = cs_mem::Block<cs_mem::DeviceAlloc>;
template <class T>
using DevBuf = cs_mem::Buf<T, cs_mem::DeviceAlloc>;
template <class T>
using PinnedBuf = cs_mem::Buf<T, cs_mem::PinnedAlloc>;

// One agent buffer: all seven columns of AgentArrays or none; view() is what the kernels take by value.
class AgentBuf {
 public:
  hipError_t alloc(uint64_t n) {
    const size_t bytes[7] = {n * sizeof(float2),   n * sizeof(float2),   n * sizeof(uint32_t), n * sizeof(uint32_t),
                             n * sizeof(uint32_t), n * sizeof(uint32_t), n * sizeof(uint32_t)};
    return cols_.alloc(bytes);
  }
  AgentArrays view() const {
    AgentArrays a{};
    a.off = static_cast<float2*>(cols_.get(0));
    a.vel = static_cast<float2*>(cols_.get(1));
    a.id = static_cast<uint32_t*>(cols_.get(2));
    a.cell = static_cast<uint32_t*>(cols_.get(3));
    a.meta = static_cast<uint32_t*>(cols_.get(4));
    a.rank = static_cast<uint32_t*>(cols_.get(5));
    a.route = static_cast<uint32_t*>(cols_.get(6));
    return a;
  }

 private:
  cs_mem::BlockSet<cs_mem::DeviceAlloc, 7> cols_;
};

#endif  // CS_DEVICE_MEM_NO_HIP

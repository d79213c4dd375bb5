// bkprim.inc — host plumbing shared by the operators built on "sort, then
// look at neighbours": top-N (bksort.inc), window (bkwin.inc), sorted dedup
// (bkdedup.inc), the post-aggregation table (bkpost.inc) and the join
// (bkjoin.inc). Included from bkgpu.hip after the pool, set_err, debug_timing
// and now_ms. Host helpers only, plus k_iota. Every rocPRIM call of the
// engine is in this file.

#include <rocprim/rocprim.hpp>

template <class T> using DevPlus = rocprim::plus<T>;
template <class T> using DevMax = rocprim::maximum<T>;

/* one checked call: keeps the status of `expr` itself (the last-error slot
 * may hold "no error" after a failing rocPRIM call or pool_alloc) */
#define BK_TRY(tag, expr, ret) do { hipError_t _e = (expr);                   \
    if (_e != hipSuccess) {                                                    \
        snprintf(g_err, sizeof g_err, "%s %s:%d %s", tag, __FILE__, __LINE__,  \
                 hipGetErrorString(_e)); return ret; } } while (0)

/* pool buffers of one operator call, returned on every exit path.
 * INVARIANT: the destructor (and scratch() when it regrows) may return
 * buffers that kernels still in flight reference. This is safe ONLY because
 * everything here runs on the null stream, every stream this engine creates
 * is blocking w.r.t. the null stream, and pool_free merely recycles within
 * this process's pool — any reuse is ordered behind the in-flight kernel by
 * stream semantics. If a non-blocking stream or an async allocator is ever
 * introduced, synchronize before a PoolBufs goes out of scope. */
struct PoolBufs {
    std::vector<void*> held;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    PoolBufs() = default;
    PoolBufs(const PoolBufs&) = delete;
    PoolBufs& operator=(const PoolBufs&) = delete;
    template <class T> hipError_t get(T** p, size_t bytes) {
        void* q = nullptr;
        hipError_t e = pool_alloc(&q, bytes ? bytes : 16);
        if (e != hipSuccess) return e;
        held.push_back(q);
        *p = (T*)q;
        return hipSuccess;
    }
    /* the one temp buffer of the dev_* calls below; grows on demand */
    void* scratch(size_t bytes) {
        if (!tmp || bytes > tmp_bytes) {
            pool_free(tmp);
            tmp = nullptr;
            tmp_bytes = 0;
            if (pool_alloc(&tmp, bytes ? bytes : 16) != hipSuccess) return nullptr;
            tmp_bytes = bytes;
        }
        return tmp;
    }
    /* hand p to the caller, who then owns it */
    template <class T> T* release(T* p) {
        held.erase(std::remove(held.begin(), held.end(), (void*)p), held.end());
        return p;
    }
    ~PoolBufs() {
        for (void* p : held) pool_free(p);
        pool_free(tmp);
    }
};

/* N events of one operator call, destroyed on every exit path */
template <int N> struct DevEvents {
    hipEvent_t e[N] = {};
    hipError_t create() {
        for (auto& x : e) {
            hipError_t r = hipEventCreate(&x);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    ~DevEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

static unsigned launch_grid(uint64_t n, unsigned per_block = 256, unsigned cap = 2048) {
    uint64_t b = (n + per_block - 1) / per_block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, cap));
}

__global__ void k_iota(uint32_t* v, uint64_t n) {
    uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gstride)
        v[i] = (uint32_t)i;
}

static void dev_iota(uint32_t* v, uint64_t n, unsigned blocks) {
    hipLaunchKernelGGL(k_iota, dim3(blocks), dim3(256), 0, 0, v, n);
}

/* rocPRIM calls: size query with the real argument types, temp from
 * bufs.scratch(), run. Iterator types pass through as the caller spells
 * them, so each call instantiates the library kernels it always did. */
template <class In, class Out, class Op>
static hipError_t dev_inclusive_scan(PoolBufs& bufs, In in, Out out, size_t n, Op op) {
    size_t bytes = 0;
    hipError_t e = rocprim::inclusive_scan(nullptr, bytes, in, out, n, op);
    if (e != hipSuccess) return e;
    void* tmp = bufs.scratch(bytes);
    if (!tmp) return hipErrorOutOfMemory;
    return rocprim::inclusive_scan(tmp, bytes, in, out, n, op);
}

template <class In, class Out, class Init, class Op>
static hipError_t dev_exclusive_scan(PoolBufs& bufs, In in, Out out, Init init,
                                     size_t n, Op op) {
    size_t bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, bytes, in, out, init, n, op);
    if (e != hipSuccess) return e;
    void* tmp = bufs.scratch(bytes);
    if (!tmp) return hipErrorOutOfMemory;
    return rocprim::exclusive_scan(tmp, bytes, in, out, init, n, op);
}

template <class KI, class KO, class VI, class VO>
static hipError_t dev_sort_pairs(PoolBufs& bufs, KI kin, KO kout, VI vin, VO vout,
                                 size_t n, unsigned begin_bit, unsigned end_bit) {
    size_t bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout,
                                             n, begin_bit, end_bit);
    if (e != hipSuccess) return e;
    void* tmp = bufs.scratch(bytes);
    if (!tmp) return hipErrorOutOfMemory;
    return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n,
                                     begin_bit, end_bit);
}

/* stable least-significant-pass-first permutation sort of n items:
 * make_key(pass, perm, keys) launches the kernel that writes the u64 sort
 * key of every position i for item perm[i] (perm == nullptr on the first
 * pass: identity); only the low bits_of_pass(pass) bits are sorted. Returns
 * the final permutation, owned by bufs, or nullptr with g_err set. */
template <class BitsOfPass, class MakeKey>
static uint32_t* dev_lsd_perm_sort(PoolBufs& bufs, uint64_t n, int npasses,
                                   BitsOfPass bits_of_pass, MakeKey make_key,
                                   unsigned iota_blocks) {
    uint32_t *pa = nullptr, *pb = nullptr;
    uint64_t *keys = nullptr, *keys_out = nullptr;
    BK_TRY("perm sort", bufs.get(&pa, n * 4), nullptr);
    BK_TRY("perm sort", bufs.get(&pb, n * 4), nullptr);
    BK_TRY("perm sort", bufs.get(&keys, n * 8), nullptr);
    BK_TRY("perm sort", bufs.get(&keys_out, n * 8), nullptr);
    dev_iota(pa, n, iota_blocks);
    for (int pass = 0; pass < npasses; pass++) {
        make_key(pass, pass == 0 ? (const uint32_t*)nullptr : pa, keys);
        BK_TRY("perm sort", hipGetLastError(), nullptr);
        BK_TRY("perm sort", dev_sort_pairs(bufs, keys, keys_out, pa, pb, (size_t)n,
                                           0, (unsigned)bits_of_pass(pass)),
               nullptr);
        std::swap(pa, pb);
    }
    return pa;
}

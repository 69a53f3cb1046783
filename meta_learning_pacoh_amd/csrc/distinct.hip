// pacoh_distinct_rows: every row of a chunk's task draws rewritten on the device as its DISTINCT tasks with their draw counts -- the
// work of engine.distinct_rows (a stable argsort plus scatters in numpy, 0.03 ms per step on the host and in front of every chunk's
// first step) as one launch behind the chunk's upload.  Integer arithmetic only: the output equals numpy's element for element.
//
// One workgroup of 256 threads per row, everything in LDS:
//   first[n_tasks]  the earliest draw position of each id (atomicMin); a draw j is its id's first occurrence iff first[id[j]] == j
//   cnt[tb]         how often the id first drawn at position j was drawn (atomicAdd at first[id]): the count sits where the flag does
//   ids[tb]         the row itself (16 bits per id): every global read is finished before the first write, so the row may be rewritten
//                   in place
// Thread t owns the consecutive positions [t * ipt, (t + 1) * ipt): a block-wide exclusive prefix sum of the threads' flag counts is
// the slot of a thread's first flagged draw, so that first occurrences keep their order.
#include "common.h"

namespace pacoh {

constexpr int DISTINCT_NT = 256;

__host__ __device__ inline size_t distinct_lds_bytes(int tb, int n_tasks) {
    // first | cnt | wave totals (4, padded to 16 B) | ids
    return (size_t)n_tasks * 4 + (size_t)tb * 4 + 16 + (size_t)tb * 2;
}

template <typename T>
__global__ __launch_bounds__(DISTINCT_NT) void distinct_rows_kernel(const long* idx, long* rows, T* __restrict__ mult,
                                                                    int32_t* __restrict__ n_act, int tb, int n_tasks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* first = reinterpret_cast<int32_t*>(smem);
    int32_t* cnt = first + n_tasks;
    int32_t* wave_tot = cnt + tb;
    uint16_t* ids = reinterpret_cast<uint16_t*>(wave_tot + 4);
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.x * tb;

    for (int i = tid; i < n_tasks; i += DISTINCT_NT) first[i] = tb;
    for (int j = tid; j < tb; j += DISTINCT_NT) cnt[j] = 0;
    __syncthreads();
    for (int j = tid; j < tb; j += DISTINCT_NT) {
        long id = idx[base + j];
        id = id < 0 ? 0 : (id >= n_tasks ? n_tasks - 1 : id);       // (the caller's ids are task numbers; no table access outside LDS)
        ids[j] = (uint16_t)id;
        atomicMin(&first[id], j);
    }
    __syncthreads();
    for (int j = tid; j < tb; j += DISTINCT_NT) atomicAdd(&cnt[first[ids[j]]], 1);

    const int ipt = (tb + DISTINCT_NT - 1) / DISTINCT_NT;
    const int lo = min(tid * ipt, tb), hi = min(lo + ipt, tb);
    int mine = 0;
    for (int j = lo; j < hi; ++j) mine += first[ids[j]] == j;
    int incl = mine;                                                 // inclusive prefix sum over the wavefront, then over the four
    const int lane = tid & (PACOH_WAVE - 1), wave = tid / PACOH_WAVE;
    for (int d = 1; d < PACOH_WAVE; d <<= 1) {
        const int up = __shfl_up(incl, d, PACOH_WAVE);
        if (lane >= d) incl += up;
    }
    if (lane == PACOH_WAVE - 1) wave_tot[wave] = incl;
    __syncthreads();                                                 // (also: every count is final)
    int slot = incl - mine, total = 0;
    for (int w = 0; w < DISTINCT_NT / PACOH_WAVE; ++w) {
        if (w < wave) slot += wave_tot[w];
        total += wave_tot[w];
    }
    for (int j = lo; j < hi; ++j) {
        if (first[ids[j]] == j) {
            rows[base + slot] = (long)ids[j];
            mult[base + slot] = (T)cnt[j];
            ++slot;
        }
    }
    const long pad = (long)ids[0];                                   // the padding: the row's first id, drawn 0 times
    for (int s = total + tid; s < tb; s += DISTINCT_NT) {
        rows[base + s] = pad;
        mult[base + s] = T(0);
    }
    if (tid == 0) n_act[blockIdx.x] = total;
}

}  // namespace pacoh

using namespace pacoh;

extern "C" int pacoh_distinct_rows(const int64_t* idx, int64_t* rows, void* mult, int32_t* n_act, int k, int tb, int n_tasks,
                                   int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (!idx || !rows || !mult || !n_act || k <= 0 || tb <= 0 || n_tasks <= 0) return PACOH_EINVAL;
    if (tb > PACOH_DISTINCT_MAX_DRAWS || n_tasks > PACOH_DISTINCT_MAX_TASKS) return PACOH_DECLINED;
    const size_t lds = distinct_lds_bytes(tb, n_tasks);              // <= 57360 bytes at the limits: no opt-in needed
    if (dtype == PACOH_F32)
        hipLaunchKernelGGL(distinct_rows_kernel<float>, dim3((unsigned)k), dim3(DISTINCT_NT), lds, (hipStream_t)stream, (const long*)idx,
                           (long*)rows, (float*)mult, n_act, tb, n_tasks);
    else
        hipLaunchKernelGGL(distinct_rows_kernel<double>, dim3((unsigned)k), dim3(DISTINCT_NT), lds, (hipStream_t)stream, (const long*)idx,
                           (long*)rows, (double*)mult, n_act, tb, n_tasks);
    return launch_status();
}

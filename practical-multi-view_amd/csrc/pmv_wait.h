// How the host waits: one implementation per kind of completion.
//   futex_wait_while / futex_wake_one   a request's owner sleeps on the request's own word, its server wakes exactly that sleeper
//   spin_for_word                       a single call spins on the word its kernel stores last into the call's result block
//   RoundSignal                         a round of launches ends with a signal kernel; its thread sleeps through most of the round
//   stage_block                         (not a wait: the copy launch in front of a solve, backend.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "pmv_device.h"
#include "pmv_mem.h"

namespace pmv {

inline void futex_wait_while(std::atomic<int>* w, int v) {
    while (w->load(std::memory_order_acquire) == v) (void)syscall(SYS_futex, (int*)w, FUTEX_WAIT_PRIVATE, v, nullptr, nullptr, 0);
}
inline void futex_wake_one(std::atomic<int>* w) { (void)syscall(SYS_futex, (int*)w, FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0); }

// PMV_BACK_WAIT=sync: the single calls wait with hipStreamSynchronize instead of spinning on their completion word (read once per process)
inline bool back_wait_by_word() { static const bool on = !(getenv("PMV_BACK_WAIT") && !strcmp(getenv("PMV_BACK_WAIT"), "sync")); return on; }

// Spins until the kernel's last store, `want`, shows in the mapped pinned `word`: the result is read as soon as that store lands.
inline hipError_t spin_for_word(hipStream_t s, volatile unsigned* word, unsigned want) {
    (void)hipStreamQuery(s);   // lets the runtime retire the commands of earlier calls now, while the GPU works on this one
    for (unsigned spins = 1;; spins++) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return hipSuccess;
        if ((spins & 0xffffu) == 0) {   // a faulted launch never signals: ask the runtime now and then
            const hipError_t e = hipStreamQuery(s);
            if (e != hipSuccess && e != hipErrorNotReady) return e;
        }
        __builtin_ia32_pause();
    }
}

// Copies `bytes` (rounded up to 16-byte granules: both blocks have that slack) from mapped pinned memory into HBM by a launch of at most
// max_blocks workgroups on the solve's own stream (backend.hip).
hipError_t stage_block(hipStream_t s, const void* mapped_src, void* dst, size_t bytes, unsigned max_blocks);

template <bool PRIO> __global__ void k_round_signal(unsigned* done, unsigned seq) {
    if (PRIO) BACKEND_PRIO();
    __threadfence_system();
    __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Completion word of a round: the round's last launch is k_round_signal, which stores the round's number into mapped pinned memory; the
// thread sleeps through 0.7 of the smoothed duration of its rounds, then looks every ~10 us (its timer slack is 1 us).
struct RoundSignal {
    Buf<unsigned> word{MEM_MAPPED};
    unsigned seq = 0;
    hipError_t init() { const hipError_t e = word.ensure(64); if (e == hipSuccess) *word = 0; return e; }
    double ema_us = 0;           // smoothed duration of the wait of a round
    struct Diag { long n_polls = 0; double t_first_sleep = 0; };
    // PRIO: the signal kernel raises its wave priority as the back-end kernels do. query_after: one hipStreamQuery once the word is seen lets
    // the runtime retire the round's commands now instead of finding them all still on its books at some later launch.
    template <bool PRIO> hipError_t signal_and_wait(hipStream_t s, bool query_after, Diag* diag = nullptr) {
        const unsigned want = ++seq;
        hipLaunchKernelGGL(k_round_signal<PRIO>, dim3(1), dim3(1), 0, s, word.dm(), want);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const auto t0 = std::chrono::steady_clock::now();
        auto done = [&] { return __atomic_load_n(word.get(), __ATOMIC_ACQUIRE) == want; };
        if (!done()) {
            const double first = 0.7 * ema_us;
            if (first > 25) {
                std::this_thread::sleep_for(std::chrono::nanoseconds((long)(first * 1e3)));
                if (diag) diag->t_first_sleep += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            }
            int looks = 0;
            while (!done()) {
                if (diag) diag->n_polls++;
                std::this_thread::sleep_for(std::chrono::microseconds(10));
                if ((++looks & 255) == 0) {   // a faulted launch never signals: ask the runtime now and then
                    e = hipStreamQuery(s);
                    if (e != hipSuccess && e != hipErrorNotReady) return e;
                }
            }
        }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        ema_us = ema_us == 0 ? us : 0.8 * ema_us + 0.2 * us;
        if (query_after) { e = hipStreamQuery(s); if (e != hipSuccess && e != hipErrorNotReady) return e; }
        return hipSuccess;
    }
};

}  // namespace pmv

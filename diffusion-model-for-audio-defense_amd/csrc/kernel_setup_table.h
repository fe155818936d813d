// Which kernel families are configured on which device: the bookkeeping of kernel_setup.hip, free of HIP so that it is tested on the host
// (tests/kernel_setup_table_main.cc).  A family's configure function acts on the calling thread's current device; the caller passes that
// device's id.
#pragma once
#include <atomic>
#include <mutex>

namespace dmad {

class SetupTable {
public:
    typedef int (*ConfigureFn)();                       // 0, or an error code that ready() hands back
    static constexpr int kMaxDevices = 64;

    // fns[i] configures the family of mask bit i; the table must outlive this object
    SetupTable(const ConfigureFn* fns, int nfamilies) : fns_(fns), n_(nfamilies) {}

    bool holds(int dev) const { return dev >= 0 && dev < kMaxDevices; }

    // Runs the configure function of every family in `mask` that device `dev` does not have yet, lowest bit first, and records each success.
    // Returns 0, or the first error: that family is not recorded, so the next call tries it again.  Once a pair is recorded a call is one
    // atomic load.  Concurrent callers of one pair run its function once (the others wait for it).
    int ready(int dev, unsigned mask) {
        if (!holds(dev)) return -1;
        if ((done_[dev].load(std::memory_order_acquire) & mask) == mask) return 0;
        std::lock_guard<std::mutex> lock(mu_);
        unsigned done = done_[dev].load(std::memory_order_relaxed);
        for (int f = 0; f < n_; ++f) {
            const unsigned bit = 1u << f;
            if (!(mask & bit) || (done & bit)) continue;
            if (int r = fns_[f]()) return r;
            done_[dev].store(done |= bit, std::memory_order_release);
        }
        return 0;
    }

private:
    const ConfigureFn* fns_;
    int n_;
    std::mutex mu_;
    std::atomic<unsigned> done_[kMaxDevices] = {};
};

}  // namespace dmad

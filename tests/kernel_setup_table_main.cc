// Host-only check of csrc/kernel_setup_table.h (SetupTable: which kernel family is configured on which device), with counting
// stand-ins for the configure functions.  Built and run by tests/test_kernel_setup_cpu.py; exit status 0 = every check held.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "kernel_setup_table.h"

namespace {

std::atomic<int> g_calls[4];
int g_fail_left = 0;            // family 2 fails this many more times, with error 719

int conf0() { ++g_calls[0]; return 0; }
int conf1() { ++g_calls[1]; return 0; }
int conf2() {
    ++g_calls[2];
    if (g_fail_left > 0) { --g_fail_left; return 719; }
    return 0;
}
std::atomic<int> g_arrived{0};
int conf3() {                   // stays inside until all eight threads are at the table's door
    ++g_calls[3];
    while (g_arrived < 8) std::this_thread::yield();
    return 0;
}
const dmad::SetupTable::ConfigureFn kFns[4] = {conf0, conf1, conf2, conf3};

int g_bad = 0;
#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) { printf("line %d: %s does not hold\n", __LINE__, #cond); ++g_bad; } \
    } while (0)
bool calls_are(int a, int b, int c, int d) { return g_calls[0] == a && g_calls[1] == b && g_calls[2] == c && g_calls[3] == d; }

}  // namespace

int main() {
    dmad::SetupTable t(kFns, 4);

    // a family is configured once per device and not again
    EXPECT(t.ready(0, 1u << 0) == 0);
    EXPECT(calls_are(1, 0, 0, 0));
    EXPECT(t.ready(0, 1u << 0) == 0);
    EXPECT(t.ready(0, 1u << 0) == 0);
    EXPECT(calls_are(1, 0, 0, 0));

    // device 1 gets its own configuration after device 0, once
    EXPECT(t.ready(1, 1u << 0) == 0);
    EXPECT(calls_are(2, 0, 0, 0));
    EXPECT(t.ready(1, 1u << 0) == 0);
    EXPECT(t.ready(0, 1u << 0) == 0);
    EXPECT(calls_are(2, 0, 0, 0));

    // a mask of several families configures each missing one exactly once (family 0 is there already on device 0)
    EXPECT(t.ready(0, (1u << 0) | (1u << 1) | (1u << 2)) == 0);
    EXPECT(calls_are(2, 1, 1, 0));
    EXPECT(t.ready(0, (1u << 0) | (1u << 1) | (1u << 2)) == 0);
    EXPECT(t.ready(0, 1u << 1) == 0);
    EXPECT(calls_are(2, 1, 1, 0));

    // a failing configure returns its error and is tried again by the next call; what succeeded before it in the mask stays done
    g_fail_left = 1;
    EXPECT(t.ready(2, (1u << 1) | (1u << 2)) == 719);
    EXPECT(calls_are(2, 2, 2, 0));
    EXPECT(t.ready(2, (1u << 1) | (1u << 2)) == 0);
    EXPECT(calls_are(2, 2, 3, 0));
    EXPECT(t.ready(2, (1u << 1) | (1u << 2)) == 0);
    EXPECT(calls_are(2, 2, 3, 0));

    // eight threads asking the same (device, family) at once run the function once, and all of them see it done
    std::atomic<int> failed{0};
    std::vector<std::thread> th;
    for (int i = 0; i < 8; ++i)
        th.emplace_back([&] {
            ++g_arrived;
            if (t.ready(3, 1u << 3) != 0) ++failed;
        });
    for (auto& x : th) x.join();
    EXPECT(failed == 0);
    EXPECT(calls_are(2, 2, 3, 1));

    // a device id outside the table is refused, nothing runs
    EXPECT(t.ready(-1, 1u << 0) != 0);
    EXPECT(t.ready(dmad::SetupTable::kMaxDevices, 1u << 0) != 0);
    EXPECT(calls_are(2, 2, 3, 1));

    if (g_bad) { printf("%d check(s) failed\n", g_bad); return 1; }
    printf("kernel_setup_table: all checks passed\n");
    return 0;
}

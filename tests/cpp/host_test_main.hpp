// The scaffold of the host layer's test programs (tests/cpp/*_tests.cpp over rivulus_amd/host/rivulus_host.hpp): case registration,
// CHECK, the shared device context and main.  Include it once, in the program's only source file.
//   <program> [--cpu] [arg]   --cpu: only the cases that need no device; arg: the program's own (a fixture or scratch directory)
// Output: "ok <name>" / "FAIL <name>: why", then "<ran> cases, <failed> failed"; exit status 0 iff all pass.
#pragma once

#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../rivulus_amd/host/rivulus_host.hpp"

#ifndef HOST_TEST_ARG_DEFAULT
#define HOST_TEST_ARG_DEFAULT "."
#endif

namespace {
struct Case {
    const char *name;
    bool needs_gpu;
    std::function<void()> fn;
};
std::vector<Case> &cases() {
    static std::vector<Case> c;
    return c;
}
struct Reg {
    Reg(const char *n, bool g, std::function<void()> f) { cases().push_back({n, g, std::move(f)}); }
};
struct Fail : std::runtime_error {
    using std::runtime_error::runtime_error;
};
#define GPU_TEST(name) \
    static void name(); \
    static Reg reg_##name(#name, true, name); \
    static void name()
#define CPU_TEST(name) \
    static void name(); \
    static Reg reg_##name(#name, false, name); \
    static void name()
#define CHECK(cond) \
    do { \
        if (!(cond)) throw Fail(std::string(__FILE__ ":") + std::to_string(__LINE__) + " CHECK(" #cond ")"); \
    } while (0)

// what() of the E that f throws, "" if it throws none
template <class E, class F>
std::string thrown(F f) {
    try {
        f();
    } catch (const E &e) {
        return e.what();
    }
    return "";
}

rivulus::ContextRef g_ctx;  // made by the first case that asks for it
[[maybe_unused]] const rivulus::ContextRef &ctx() {
    if (!g_ctx) g_ctx = std::make_shared<rivulus::Context>(0);
    return g_ctx;
}
[[maybe_unused]] std::string g_arg = HOST_TEST_ARG_DEFAULT;
}  // namespace

int main(int argc, char **argv) {
    bool cpu_only = false;
    for (int i = 1; i < argc; ++i) {
        if (std::string(argv[i]) == "--cpu") cpu_only = true;
        else g_arg = argv[i];
    }
    int failed = 0, ran = 0;
    for (auto &c : cases()) {
        if (cpu_only && c.needs_gpu) continue;
        ++ran;
        try {
            c.fn();
            std::printf("ok %s\n", c.name);
        } catch (const std::exception &e) {
            std::printf("FAIL %s: %s\n", c.name, e.what());
            ++failed;
        }
        std::fflush(stdout);
    }
    g_ctx.reset();
    std::printf("%d cases, %d failed\n", ran, failed);
    return failed ? 1 : 0;
}

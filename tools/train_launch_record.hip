// What do the launchers of the five ConvNeXt training operators launch?  No GPU: the host code of a tree's units is compiled against a
// recording stand-in for hipLaunchKernelGGL, so every launch prints (kernel instantiation, grid, block, dynamic LDS, the integral kernel
// arguments) instead of running.  Two trees that print the same table launch the same kernels the same way.
//
//   for u in dwln_train block_tail lncf_train down_train pw_mlp; do
//     hipcc --cuda-host-only -O1 -std=c++17 -I TREE/unicorn_amd/csrc -DRECORD_UNIT="\"$u.hip\"" -c tools/train_launch_record.hip -o $u.o; done
//   hipcc --cuda-host-only -O1 -std=c++17 -I TREE/unicorn_amd/csrc -c tools/train_launch_record.hip -o driver.o
//   hipcc driver.o dwln_train.o block_tail.o lncf_train.o down_train.o pw_mlp.o -o record && ./record > table.txt
//
// With RECORD_UNIT this file is that unit with the launch macro replaced; without, the driver that walks the shapes.  Pointers are made up
// (nothing is dereferenced on the host).  profiles/train_plan_shared.txt holds a comparison made this way.
#include "common.h"
#include "kernels.h"

#include <string>
#include <type_traits>
#include <typeinfo>

void record_launch(const char* mangled, dim3 grid, dim3 block, size_t lds, const std::string& args);

#ifdef RECORD_UNIT
struct DwlnRJob;                                // train_ops.h, which launches too: it is read below, after the launch macro is replaced
template <auto K>
struct KernelName {};                           // its mangled name holds that of the instantiation: the driver demangles it
template <typename A, typename = void>
struct HasStripPlan : std::false_type {};
template <typename A>
struct HasStripPlan<A, std::void_t<decltype(A::CGp)>> : std::true_type {};
template <typename A>
static void record_arg(std::string& s, const A& a) {
    if constexpr (std::is_integral_v<A>) s += " " + std::to_string(a);
    else if constexpr (HasStripPlan<A>::value)                      // DwlnK carries its plan by value
        s += " CG=" + std::to_string(a.CG) + " CGp=" + std::to_string(a.CGp) + " NS=" + std::to_string(a.NS) + " segs=" + std::to_string(a.segs) +
             " nstrips=" + std::to_string(a.nstrips);
}
static void record_arg(std::string& s, const DwlnRJob& j);
template <typename... A>
static std::string record_args(const A&... a) {
    std::string s;
    (record_arg(s, a), ...);
    return s;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    ((void)(stream), record_launch(typeid(KernelName<kernel>).name(), grid, block, lds, record_args(__VA_ARGS__)))
#include "train_ops.h"
static void record_arg(std::string& s, const DwlnRJob& j) {         // the partials a reduce job reads: byte offset in the workspace, rows, columns
    s += " job(" + (j.blocks ? std::to_string(reinterpret_cast<uintptr_t>(j.part) - 0x10000) : std::string("-")) + " R=" + std::to_string(j.R) +
         " N=" + std::to_string(j.N) + " n1=" + std::to_string(j.n1) + " blocks=" + std::to_string(j.blocks) + ")";
}
#include RECORD_UNIT

#else
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>

std::atomic<int> g_uni_variant_trace{0};
void uni_variant_record(const char*, ...) {}
void uni_set_error(const char* fmt, ...) {
    if (std::strstr(fmt, "%s:%d: %s -> %s")) return;               // UNI_CHECK_HIP(hipGetLastError()): there is no device here
    va_list ap;
    va_start(ap, fmt);
    std::printf("    refused: ");
    std::vprintf(fmt, ap);
    std::printf("\n");
    va_end(ap);
}
void record_launch(const char* mangled, dim3 grid, dim3 block, size_t lds, const std::string& args) {
    int status = 0;
    char* plain = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);       // "KernelName<&ln_cl_kernel<float, _Float16, 8, 3, 1, DownIO>(LnClK<float>, DownIO, ...)>"
    std::string name = status == 0 ? plain : mangled;
    std::free(plain);
    if (name.rfind("KernelName<&", 0) == 0) name = name.substr(12, name.size() - 13);
    std::printf("    %s grid (%u, %u, %u) block %u lds %zu args%s\n", name.c_str(), grid.x, grid.y, grid.z, block.x, lds, args.c_str());
}

template <typename T>
static T* fake() { return reinterpret_cast<T*>(0x10000); }
static const int CS[] = {4, 8, 96, 100, 256, 260, 384, 500, 1000, 1536, 2044, 2048};      // 256, 260: the last regs=32 width of lncf and the first streamed one
struct Map { int B, H, W; };
// tests/train_plans.py MAP and MAP_DW, then maps with more work units than a launch has blocks
static const Map MAPS[] = {{2, 3, 7}, {2, 5, 11}, {1, 65, 65}, {2, 200, 320}, {7, 300, 300}};
static const char* const DT[] = {"T", "f16", "bf16"};

template <typename T>
static void run(const char* tn) {
    const size_t big = (size_t)1 << 60;
    for (const Map& m : MAPS)
        for (int C : CS) {
            for (int dt = 0; dt < (sizeof(T) == 8 ? 1 : 3); ++dt)
                for (int nchw = 0; nchw < 2; ++nchw) {
                    std::printf("lncf<%s> x=%s %s B=%d H=%d W=%d C=%d\n", tn, DT[dt], nchw ? "nchw" : "cl", m.B, m.H, m.W, C);
                    const LncfArgs<T> a{fake<void>(), dt, nchw, fake<T>(), fake<T>(), 1e-6, m.B, m.H, m.W, C};
                    launch_lncf_train_fwd<T>(a, fake<T>(), fake<T>(), nullptr);
                    launch_lncf_train_bwd<T>(a, fake<T>(), fake<T>(), fake<void>(), fake<T>(), fake<T>(), fake<void>(), big, nullptr);
                    launch_lncf_train_bwd<T>(a, fake<T>(), fake<T>(), fake<void>(), nullptr, nullptr, nullptr, 0, nullptr);
                    std::printf("block_tail<%s> y=%s %s B=%d H=%d W=%d C=%d\n", tn, DT[dt], nchw ? "nchw" : "cl", m.B, m.H, m.W, C);
                    const BtArgs<T> b{fake<void>(), dt, fake<T>(), nchw, fake<T>(), fake<T>(), m.B, m.H, m.W, C};
                    launch_block_tail_fwd<T>(b, fake<T>(), nullptr);
                    launch_block_tail_bwd<T>(b, fake<void>(), fake<T>(), fake<void>(), big, nullptr);
                }
            // downsample_ln: x and A of one element type, and fp32 x into a bf16 A
            for (int dt = 0; dt < (sizeof(T) == 8 ? 1 : 3); ++dt)
                for (int ad = dt; ad < (sizeof(T) == 8 ? 1 : 3); ad += 2) {
                    std::printf("down<%s> x=%s a=%s B=%d H=%d W=%d C=%d\n", tn, DT[dt], DT[ad], m.B, m.H, m.W, C);
                    const DownArgs<T> a{fake<void>(), dt, ad, fake<T>(), fake<T>(), 1e-6, m.B, m.H, m.W, C};
                    launch_down_train_fwd<T>(a, 0, fake<void>(), fake<T>(), nullptr);
                    launch_down_train_fwd<T>(a, 1, fake<void>(), fake<T>(), nullptr);
                    launch_down_train_bwd<T>(a, fake<T>(), fake<void>(), fake<void>(), fake<T>(), fake<T>(), fake<void>(), big, nullptr);
                    launch_down_train_bwd<T>(a, fake<T>(), fake<void>(), fake<void>(), nullptr, nullptr, nullptr, 0, nullptr);
                }
            std::printf("dwln<%s> B=%d H=%d W=%d C=%d\n", tn, m.B, m.H, m.W, C);
            const DwlnArgs<T> d{fake<T>(), fake<T>(), fake<T>(), fake<T>(), fake<T>(), 1e-6, m.B, m.H, m.W, C};
            launch_dwln_train_fwd<T>(d, fake<T>(), fake<T>(), nullptr);
            launch_dwln_train_bwd<T>(d, fake<T>(), fake<T>(), fake<T>(), fake<T>(), fake<T>(), fake<T>(), fake<T>(), fake<void>(), big, nullptr);
        }
    // pw_mlp: the four shapes of tests/pw_mlp_ref.py CASES and one stage of a full-size step
    static const int PW[][3] = {{15, 16, 4}, {42, 96, 24}, {42, 100, 12}, {96, 192, 48}, {128000, 768, 192}};
    for (const auto& s : PW)
        for (int dt = 0; dt < (sizeof(T) == 8 ? 1 : 3); ++dt) {
            std::printf("pw_mlp<%s> h=%s M=%d Hd=%d Co=%d\n", tn, DT[dt], s[0], s[1], s[2]);
            launch_pw_mlp_act_fwd<T>(fake<void>(), dt, s[0], s[1], fake<void>(), nullptr);
            const PwBwdArgs<T> a{fake<void>(), fake<void>(), dt, s[0], s[1], fake<void>(), fake<void>(), fake<T>(), fake<void>(), s[2], fake<T>()};
            launch_pw_mlp_act_bwd<T>(a, fake<void>(), big, nullptr);
        }
}

int main() {
    run<float>("float");
    run<double>("double");
    return 0;
}
#endif

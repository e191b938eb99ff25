// rank_launch.hip -- what a launch of rank_loop_kernel asks the runtime, once for every kernels translation unit: the dynamic-LDS limit of a build and
// how many of its workgroups a CU holds.  The builds are named in kernels.hip (with_rank_kernel); here a build is a `const void *`.
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#include "device_types.hpp"
#include "launch.hpp"

namespace mcrat {

// What the runtime has been asked about a kernel on a device.  The dynamic-LDS limit is the kernel's, not a context's: every context of the process
// launches the same kernel, so the note is the process's (a context's own note would go stale when another context set a smaller size).  The limit is
// only ever raised -- a launch may use less than the limit -- and the occupancy is kept for the LDS size it was asked for last.
struct KernelNote { const void *kernel; int device, max_dyn, occ_dyn, per_cu; };
static std::mutex g_kernel_notes_lock;
static std::vector<KernelNote> g_kernel_notes;
static KernelNote &kernel_note(const void *kernel, int device)      // (with the lock held)
{
    for (KernelNote &k : g_kernel_notes)
        if (k.kernel == kernel && k.device == device) return k;
    g_kernel_notes.push_back(KernelNote{kernel, device, -1, -1, 0});
    return g_kernel_notes.back();
}
static int launch_device(const RankDeviceInfo *dev)
{
    int d = 0;
    if (dev) return dev->device;
    if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; }
    return d;
}
// hipFuncSetAttribute(.., hipFuncAttributeMaxDynamicSharedMemorySize, dyn), unless the kernel's limit on this device is known to be at least dyn
static hipError_t allow_dynamic_lds(const void *kernel, int device, int dyn)
{
    std::lock_guard<std::mutex> hold(g_kernel_notes_lock);
    KernelNote &k = kernel_note(kernel, device);
    if (k.max_dyn >= dyn) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    if (e == hipSuccess) k.max_dyn = dyn;
    return e;
}
// workgroups of `threads` threads and `dyn` bytes of dynamic LDS that one CU holds (0: the runtime would not say)
static int resident_per_cu(const void *kernel, int device, int threads, size_t dyn)
{
    std::lock_guard<std::mutex> hold(g_kernel_notes_lock);
    KernelNote &k = kernel_note(kernel, device);
    if (k.occ_dyn == (int)dyn) return k.per_cu;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, dyn) != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); return 0; }
    k.occ_dyn = (int)dyn; k.per_cu = per_cu;
    return per_cu;
}

int rank_launch_grid(const void *kernel, const RankLaunch &rl, const RankFormPlan &plan)
{
    const int device = plan.form.resident ? launch_device(rl.dev) : 0;
    // static + dynamic LDS may exceed the 64 KiB default: the kernel must be told
    if (plan.form.resident && allow_dynamic_lds(kernel, device, (int)plan.lds_bytes) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (!plan.form.queue) return rl.n_ranks;
    int cus = rl.dev ? rl.dev->cus : 0;
    const int per_cu = resident_per_cu(kernel, device, plan.form.threads, plan.lds_bytes);
    if (cus <= 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); cus = 0; }
    return rank_queue_grid(rl.n_open, per_cu, cus);
}

}  // namespace mcrat

// ------------------------------------------------------------------------------------------------
// multi-GPU gather of results over RCCL (single process, one handle per GPU) -- SURVEY 8(e)
// ------------------------------------------------------------------------------------------------
#include "batch.h"

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is dlopen()ed by dsp_gather_results, never linked

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::vector<int> devs;               // communicators are cached for the last device list
    std::vector<ncclComm_t> comms;
    std::mutex mu;
};
Rccl g_rccl;

void rccl_load() {
    if (g_rccl.lib) return;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        g_rccl.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) throw std::runtime_error(std::string("cannot load librccl: ") + dlerror());
#define RCCL_SYM(field, sym)                                                                  \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(g_rccl.lib, #sym));      \
    if (!g_rccl.field) throw std::runtime_error("librccl lacks " #sym)
    RCCL_SYM(CommInitAll, ncclCommInitAll);
    RCCL_SYM(CommDestroy, ncclCommDestroy);
    RCCL_SYM(GroupStart, ncclGroupStart);
    RCCL_SYM(GroupEnd, ncclGroupEnd);
    RCCL_SYM(Gather, ncclGather);
    RCCL_SYM(GetErrorString, ncclGetErrorString);
#undef RCCL_SYM
}

#define RCCL_TRY(expr)                                                                                           \
    do {                                                                                                         \
        ncclResult_t r_ = (expr);                                                                                \
        if (r_ != ncclSuccess) throw std::runtime_error(std::string(#expr " failed: ") + g_rccl.GetErrorString(r_)); \
    } while (0)

}  // namespace

namespace {

// One ncclGather of n_handles equal blocks (uneven shards padded to the largest) to handles[0]'s GPU, then ONE copy to the host.
// src[i]: n_objects[i] x DSP_RESULT_WIDTH floats, on the host (src_on_device false) or already on handles[i]'s device.
// Every handle's mutex is held for the whole call, taken in address order (two concurrent gathers over overlapping handle sets
// cannot deadlock, and a dsp_batch_run on any of the handles from its own host thread -- SURVEY 8(e)'s one-thread-per-device
// model -- waits instead of interleaving with the collective on that handle's stream).
void gather_impl(dsp_handle* const* handles, int n_handles, const float* const* src, bool src_on_device, const int32_t* n_objects, float* out,
                 dsp_batch* const* batches = nullptr) {
    std::vector<dsp_handle*> order(handles, handles + n_handles);
    std::sort(order.begin(), order.end());
    if (std::adjacent_find(order.begin(), order.end()) != order.end()) throw std::invalid_argument("dsp_gather_results: the same handle twice");
    std::vector<std::unique_lock<std::mutex>> locks;
    for (dsp_handle* h : order) locks.emplace_back(h->mu);
    if (batches)
        for (int i = 0; i < n_handles; ++i)
            if (batches[i]->iters_run <= 0) throw std::invalid_argument("dsp_gather_batch_results: a batch has not been run");
    std::lock_guard<std::mutex> lock(g_rccl.mu);
    rccl_load();
    std::vector<int> devs(n_handles);
    int n_max = 0;
    for (int i = 0; i < n_handles; ++i) {
        devs[i] = handles[i]->device;
        n_max = std::max(n_max, (int)n_objects[i]);
        for (int j = 0; j < i; ++j)
            if (devs[j] == devs[i]) throw std::invalid_argument("dsp_gather_results: one handle per GPU (two handles share a device)");
    }
    if (devs != g_rccl.devs) {
        for (ncclComm_t c : g_rccl.comms) (void)g_rccl.CommDestroy(c);
        g_rccl.comms.assign(n_handles, nullptr);
        g_rccl.devs.clear();
        RCCL_TRY(g_rccl.CommInitAll(g_rccl.comms.data(), n_handles, devs.data()));
        g_rccl.devs = devs;
    }
    const size_t block = (size_t)std::max(n_max, 1) * DSP_RESULT_WIDTH;     // uneven shards are padded to the largest
    std::vector<DevBuf<float>> send(n_handles);
    DevBuf<float> recv;
    for (int i = 0; i < n_handles; ++i) {
        HIP_TRY(hipSetDevice(devs[i]));
        send[i].alloc(block);
        HIP_TRY(hipMemsetAsync(send[i].p, 0, block * 4, handles[i]->stream));
        if (n_objects[i])
            HIP_TRY(hipMemcpyAsync(send[i].p, src[i], (size_t)n_objects[i] * DSP_RESULT_WIDTH * 4,
                                   src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, handles[i]->stream));
        if (i == 0) recv.alloc(block * n_handles);
    }
    {
        RCCL_TRY(g_rccl.GroupStart());       // the ONE collective of the path: every GPU's block to the first handle's GPU, over xGMI
        struct GroupGuard {                  // an exception between Start and End must not leave the group open for the rest of the process
            bool open = true;
            ~GroupGuard() { if (open) (void)g_rccl.GroupEnd(); }
        } guard;
        for (int i = 0; i < n_handles; ++i)
            RCCL_TRY(g_rccl.Gather(send[i].p, i == 0 ? recv.p : nullptr, block, ncclFloat, 0, g_rccl.comms[i], handles[i]->stream));
        guard.open = false;
        RCCL_TRY(g_rccl.GroupEnd());
    }
    for (int i = 0; i < n_handles; ++i) {
        HIP_TRY(hipSetDevice(devs[i]));
        HIP_TRY(hipStreamSynchronize(handles[i]->stream));
    }
    HIP_TRY(hipSetDevice(devs[0]));
    std::vector<float> host(block * n_handles);
    HIP_TRY(hipMemcpy(host.data(), recv.p, host.size() * 4, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (int i = 0; i < n_handles; ++i) {
        memcpy(out + o, host.data() + (size_t)i * block, (size_t)n_objects[i] * DSP_RESULT_WIDTH * 4);
        o += (size_t)n_objects[i] * DSP_RESULT_WIDTH;
    }
}

template <class F>
int guarded_nolock(dsp_handle* err_to, F f) {      // guarded() without taking a handle mutex (the callee takes several)
    try {
        f();
        return DSP_OK;
    } catch (const std::exception&) {
        std::string msg;
        const int rc = translate_error(msg);
        std::lock_guard<std::mutex> l(err_to->mu);
        err_to->err = msg;
        return rc;
    }
}

}  // namespace

extern "C" int dsp_gather_results(dsp_handle* const* handles, int32_t n_handles, const float* const* results, const int32_t* n_objects,
                                  float* out) {
    if (!handles || n_handles < 1 || !results || !n_objects || !out) return DSP_E_ARG;
    for (int i = 0; i < n_handles; ++i)
        if (!handles[i] || n_objects[i] < 0 || (n_objects[i] > 0 && !results[i])) return DSP_E_ARG;
    return guarded_nolock(handles[0], [&] { gather_impl(handles, n_handles, results, false, n_objects, out); });
}

extern "C" int dsp_gather_batch_results(dsp_batch* const* batches, int32_t n_batches, float* out) {
    if (!batches || n_batches < 1 || !out) return DSP_E_ARG;
    std::vector<dsp_handle*> handles(n_batches);
    std::vector<const float*> src(n_batches);
    std::vector<int32_t> n_obj(n_batches);
    std::vector<std::unique_ptr<BatchRef>> refs;          // every token resolved, every handle pinned for the whole call
    std::vector<dsp_batch*> impl(n_batches);
    for (int i = 0; i < n_batches; ++i) {
        refs.emplace_back(new BatchRef(batches[i]));
        if (!refs.back()->b) return DSP_E_ARG;
        impl[i] = refs.back()->b;
        handles[i] = impl[i]->h;
        src[i] = impl[i]->out_packed.p;
        n_obj[i] = impl[i]->n_obj;
    }
    return guarded_nolock(handles[0], [&] {
        // "has it been run" is checked by gather_impl once every handle's mutex is held: a dsp_batch_run on another host thread (the
        // documented one-thread-per-GPU model) may be writing iters_run right now
        gather_impl(handles.data(), n_batches, src.data(), true, n_obj.data(), out, impl.data());
    });
}

extern "C" int dsp_batch_results_packed_dev(dsp_batch* tok, float* dst_dev) {
    BatchRef ref_(tok);
    dsp_batch* const b = ref_.b;
    if (!b || !dst_dev) return DSP_E_ARG;
    return guarded(b->h, [&] {
        if (b->iters_run <= 0) throw std::invalid_argument("dsp_batch_results_packed_dev: the batch has not been run");
        HIP_TRY(hipSetDevice(b->h->device));
        HIP_TRY(hipMemcpyAsync(dst_dev, b->out_packed.p, (size_t)b->n_obj * DSP_RESULT_WIDTH * 4, hipMemcpyDeviceToDevice, b->h->stream));
        HIP_TRY(hipStreamSynchronize(b->h->stream));
    });
}

extern "C" void dsp_pack_results(int32_t n, const float* t_cam_obj, const float* codes, const float* loss, const int32_t* status, float* packed) {
    for (int32_t i = 0; i < n; ++i) {
        float* row = packed + (size_t)i * DSP_RESULT_WIDTH;
        memcpy(row, t_cam_obj + (size_t)i * 16, 64);
        memcpy(row + 16, codes + (size_t)i * CODE_LEN, CODE_LEN * 4);
        row[80] = loss[i];
        row[81] = (float)status[i];
    }
}

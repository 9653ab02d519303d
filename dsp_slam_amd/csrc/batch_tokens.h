// Batch tokens: the slot table behind dsp_batch_create / dsp_batch_destroy / dsp_destroy, the pin guard of a call on a batch, and the two
// retire-then-wait sequences.  Standard library only, and written against the members it uses -- Batch: `h` (its handle) and `pins`;
// handle: `pins` and `mu` -- so that tests/host/token_driver.cpp runs it on stand-in types under a host sanitizer.
#pragma once
#include <atomic>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

namespace batch_tokens __attribute__((visibility("hidden"))) {      // the table's static members are no exports of the library

// What dsp_batch_create hands out is NOT the address of the batch object but an opaque, generation-tagged token: slot index and the slot's
// generation packed into the pointer value (bit 0 set: never a valid object address).  A slot's generation advances when its batch goes away,
// so a token that outlived its batch -- dsp_destroy of the handle took the batch with it, or it was destroyed twice -- resolves to nothing,
// even after the allocator has reused the batch's address for another handle's batch (the use-after-free a raw-pointer registry allowed).
// A call that resolves a token PINS the batch's handle until it returns: dsp_destroy first retires the handle's tokens (no new call can
// reach the handle through them), then waits for the pinned calls in flight, and only then frees anything -- so the two destroy calls are
// safe in either order and from any thread (a garbage collector's finaliser thread included).
constexpr int TOKEN_IDX_BITS = 20;

template <class Batch>
struct Table {
    struct BatchSlot { uint64_t gen = 1; Batch* impl = nullptr; };
    static inline std::mutex g_live_mu;
    static inline std::vector<BatchSlot> g_slots;
    static inline std::vector<uint32_t> g_free_slots;

    static Batch* token_of(uint32_t idx, uint64_t gen) {
        return reinterpret_cast<Batch*>((uintptr_t)((gen << (TOKEN_IDX_BITS + 1)) | ((uint64_t)idx << 1) | 1u));
    }
    static Batch* register_batch(Batch* impl) {
        std::lock_guard<std::mutex> lock(g_live_mu);
        uint32_t idx;
        if (!g_free_slots.empty()) { idx = g_free_slots.back(); g_free_slots.pop_back(); }
        else {
            if (g_slots.size() >= ((size_t)1 << TOKEN_IDX_BITS)) throw std::runtime_error("too many live batches");
            idx = (uint32_t)g_slots.size();
            g_slots.emplace_back();
        }
        g_slots[idx].impl = impl;
        return token_of(idx, g_slots[idx].gen);
    }
    // (g_live_mu held) the batch a token stands for, or nullptr for a stale / foreign value; slot_out: its slot
    static Batch* resolve_locked(const Batch* token, uint32_t* slot_out = nullptr) {
        const uintptr_t v = reinterpret_cast<uintptr_t>(token);
        if (!(v & 1u)) return nullptr;
        const uint32_t idx = (uint32_t)((v >> 1) & (((uintptr_t)1 << TOKEN_IDX_BITS) - 1));
        const uint64_t gen = (uint64_t)v >> (TOKEN_IDX_BITS + 1);
        if (idx >= g_slots.size() || g_slots[idx].gen != gen || !g_slots[idx].impl) return nullptr;
        if (slot_out) *slot_out = idx;
        return g_slots[idx].impl;
    }
    static void retire_slot_locked(uint32_t idx) {
        g_slots[idx].impl = nullptr;
        g_slots[idx].gen++;
        g_free_slots.push_back(idx);
    }
    // resolves a token for the duration of one call and keeps the batch's handle alive meanwhile
    struct BatchRef {
        Batch* b = nullptr;
        explicit BatchRef(const Batch* token) {
            std::lock_guard<std::mutex> lock(g_live_mu);
            b = resolve_locked(token);
            if (b) { b->h->pins.fetch_add(1); b->pins.fetch_add(1); }
        }
        ~BatchRef() { if (b) { auto* h = b->h; b->pins.fetch_sub(1); h->pins.fetch_sub(1); } }
        BatchRef(const BatchRef&) = delete;
        BatchRef& operator=(const BatchRef&) = delete;
    };

    // dsp_batch_destroy: retire the token, wait for the calls pinned on the batch, then free_batch(b, h) under the handle's lock (the
    // handle is pinned meanwhile).  A NULL or stale token, or one dsp_destroy of its handle took already, is a no-op.
    template <class Free>
    static void destroy_batch(const Batch* tok, Free free_batch) {
        Batch* b;
        decltype(b->h) h;
        {
            std::lock_guard<std::mutex> live(g_live_mu);
            uint32_t slot = 0;
            b = resolve_locked(tok, &slot);
            if (!b) return;                      // NULL, stale, or dsp_destroy of its handle took it already
            retire_slot_locked(slot);
            h = b->h;
            h->pins.fetch_add(1);                // the handle outlives this call (dsp_destroy waits for pinned calls)
        }
        while (b->pins.load() > 0) std::this_thread::yield();      // a call on this batch from another thread that resolved the token before it was retired
        {
            std::lock_guard<std::mutex> lock(h->mu);      // its device blocks and events go back to the handle's pools
            free_batch(b, h);
        }
        h->pins.fetch_sub(1);
    }

    // dsp_destroy: retire every token of the handle, wait for the calls pinned on it and for the call holding its lock, then
    // free_all(orphans): the handle's batches that were still alive, for the caller to free with the handle.
    template <class Handle, class Free>
    static void destroy_handle(Handle* h, Free free_all) {
        if (!h) return;
        std::vector<Batch*> orphans;
        {
            std::lock_guard<std::mutex> lock(g_live_mu);
            for (uint32_t i = 0; i < g_slots.size(); ++i)
                if (g_slots[i].impl && g_slots[i].impl->h == h) { orphans.push_back(g_slots[i].impl); retire_slot_locked(i); }
        }
        while (h->pins.load() > 0) std::this_thread::yield();      // calls that resolved one of its tokens before they were retired
        { std::lock_guard<std::mutex> lock(h->mu); }                // ... and whatever call on the handle itself is still running
        free_all(orphans);
    }
};

}  // namespace batch_tokens

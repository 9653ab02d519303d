// Stand-alone driver for dsp_slam_amd/csrc/batch_tokens.h on stand-in handle and batch types (tests/test_token_table.py builds it with
// -fsanitize=thread and with -fsanitize=address,undefined).  No HIP, no libdspgn.  Exit status 0 = every check held; a sanitizer report
// makes the status non-zero by itself.
#include "batch_tokens.h"

#include <cstdio>
#include <cstdlib>

struct Handle {
    std::mutex mu;
    std::atomic<int> pins{0};
    long touched = 0;
};
struct Batch {
    Handle* h = nullptr;
    std::atomic<int> pins{0};
    long touched = 0;
};
using Tokens = batch_tokens::Table<Batch>;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

// the library's entry points, on the stand-ins: what dsp_batch_create / a call on a batch / dsp_batch_destroy / dsp_destroy do with a token
static Batch* create(Handle* h) {
    Batch* b = new Batch;
    b->h = h;
    return Tokens::register_batch(b);
}
static bool touch(Batch* tok) {         // like guarded(b->h, ...): resolve and pin, take the handle's lock, write the batch and its handle
    Tokens::BatchRef ref(tok);
    if (!ref.b) return false;
    std::lock_guard<std::mutex> lock(ref.b->h->mu);
    ref.b->touched++;
    ref.b->h->touched++;
    return true;
}
static void destroy_batch(Batch* tok) {
    Tokens::destroy_batch(tok, [](Batch* b, Handle* h) { h->touched++; delete b; });
}
static void destroy_handle(Handle* h) {
    Tokens::destroy_handle(h, [h](const std::vector<Batch*>& orphans) {
        for (Batch* b : orphans) delete b;
        delete h;
    });
}
static Batch* resolve(Batch* tok) {
    std::lock_guard<std::mutex> lock(Tokens::g_live_mu);
    return Tokens::resolve_locked(tok);
}

static void single_threaded() {
    Handle* h = new Handle;
    Batch* t1 = create(h);
    CHECK(((uintptr_t)t1 & 1u) == 1u);
    Batch* b1 = resolve(t1);
    CHECK(b1 && b1->h == h);                          // a token resolves to its batch
    CHECK(touch(t1) && b1->touched == 1 && h->touched == 1);
    destroy_batch(t1);
    CHECK(!resolve(t1) && !touch(t1));                // after retire it resolves to nothing
    Batch* t2 = create(h);                            // the slot is reused ...
    CHECK(t2 != t1 && (((uintptr_t)t2 >> 1) & 0xFFFFF) == (((uintptr_t)t1 >> 1) & 0xFFFFF));
    CHECK(!resolve(t1) && resolve(t2));               // ... the old token still resolves to nothing, the new one resolves
    CHECK(!resolve(nullptr));
    CHECK(!resolve(resolve(t2)));                     // an even (pointer-like) value: the object's own address
    CHECK(!resolve(reinterpret_cast<Batch*>((uintptr_t)((1ull << 21) | (0xFFFFFull << 1) | 1u))));   // an index beyond the table
    destroy_batch(t2);
    destroy_batch(t2);                                // destroying a batch twice is a no-op
    destroy_batch(nullptr);
    Handle* other = new Handle;
    Batch* ta = create(h);
    Batch* tb = create(h);
    Batch* tc = create(other);
    destroy_handle(h);                                // retires every token of that handle and none of another handle's
    CHECK(!resolve(ta) && !resolve(tb) && resolve(tc) && touch(tc));
    destroy_batch(ta);                                // a later batch-destroy of such a token is a no-op
    CHECK(!touch(tb));
    destroy_handle(other);
    CHECK(!resolve(tc));
    destroy_handle(static_cast<Handle*>(nullptr));
}

// 8 threads, a fixed seeded number of operations each, over 4 handle places.  A place's handle is swapped for a fresh one under the
// place's lock (as a caller would not create batches on a handle it is destroying) and destroyed OUTSIDE it, so resolves, touches and
// batch-destroys through tokens of that handle race with its destruction.
constexpr int N_THREADS = 8, N_PLACES = 4, N_OPS = 60000, BAG = 256;
static std::mutex place_mu[N_PLACES];
static Handle* place[N_PLACES];
static std::mutex bag_mu;
static Batch* bag[BAG];

static void worker(int tid) {
    uint32_t x = 2463534242u + 7919u * (uint32_t)tid;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int op = 0; op < N_OPS; ++op) {
        const uint32_t r = rnd() % 100, slot = rnd() % BAG;
        Batch* tok;
        { std::lock_guard<std::mutex> l(bag_mu); tok = bag[slot]; }
        if (r < 30) {                                 // register
            const int p = (int)(rnd() % N_PLACES);
            Batch* t;
            { std::lock_guard<std::mutex> l(place_mu[p]); t = create(place[p]); }
            Batch* old;
            { std::lock_guard<std::mutex> l(bag_mu); old = bag[slot]; bag[slot] = t; }
            destroy_batch(old);                       // (keeps the table from growing: stale or NULL is a no-op)
        } else if (r < 80) {                          // resolve and touch through the pin guard
            touch(tok);
        } else if (r < 97) {                          // batch-destroy; the token stays in the bag as a stale one
            destroy_batch(tok);
        } else {                                      // handle-destroy
            const int p = (int)(rnd() % N_PLACES);
            Handle* old;
            { std::lock_guard<std::mutex> l(place_mu[p]); old = place[p]; place[p] = new Handle; }
            destroy_handle(old);
        }
    }
}

int main() {
    single_threaded();
    for (auto& h : place) h = new Handle;
    std::vector<std::thread> threads;
    for (int t = 0; t < N_THREADS; ++t) threads.emplace_back(worker, t);
    for (auto& t : threads) t.join();
    for (auto& h : place) destroy_handle(h);
    for (Batch* tok : bag) CHECK(!resolve(tok));
    for (const auto& s : Tokens::g_slots) CHECK(!s.impl);
    printf("ok: %zu slots\n", Tokens::g_slots.size());
    return 0;
}

// graph_guard.h -- the bookkeeping that ties a captured graph (j2k_ctx_capture_begin / _end, j2k_graph_launch) to the device memory it recorded,
// without any HIP in it: tests/graph_guard_main.cpp drives it on the CPU with scripted histories.
//
// A graph replays raw device pointers.  Three things free such pointers while the graph is alive, and each makes it STALE:
//   (a) a staging slot of the context that the capture used is reallocated (stage_reserve grows it);
//   (b) a growable buffer of a plan whose calls the capture recorded is reallocated (ensure_sized: d_cl_dense, d_host_io, d_host_pix);
//   (c) such a plan is destroyed.
// j2k_graph_launch refuses a stale graph before anything is launched.
//
// What is kept.  Per context: a generation per staging slot, bumped where the slot is reallocated, and one entry per LIVE plan, serial -> the
// plan's generation, bumped where a plan-owned buffer is reallocated.  A plan's serial is taken from a counter of the context that only goes up:
// an address comes back after a free, a serial does not, so a new plan at a destroyed plan's address is another plan.  A destroyed plan's entry
// is erased; since no later plan gets its serial, "no entry" IS the tombstone and the table stays as small as the set of live plans.
// While the context captures, slot_used() / plan_used() note what the recorded calls touch (stage_reserve runs on every call, also when the slot
// is big enough; every plan entry point of the C ABI notes its plan first thing); capture_end() snapshots the generations of what was noted;
// verdict() compares.  Nothing else enters: a slot the capture did not reserve, a plan it did not call, a plan of another context cannot stale a graph.
//
// The counters are uint64_t and compared for EQUALITY, so a stale graph could read as valid again only after exactly 2^64 (or a multiple)
// reallocations of the one slot or plan buffer.  Each of those is a stream synchronisation, a hipFree and a hipMalloc -- at a microsecond apiece
// 2^64 of them take 580 000 years.  No number of bumps below 2^64 brings a generation back to a snapshot's (tests/graph_guard_main.cpp: "wrap").
// The serial counter is 64 bits wide for the same reason: it is never reset and a context does not make 2^64 plans.
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace j2k {

struct GraphGuard {
    static constexpr int SLOTS = 5;
    enum Verdict { VALID = 0, STALE_SLOT = 1, STALE_PLAN_BUFFER = 2, STALE_PLAN_DESTROYED = 3 };   // the causes (a), (b), (c)

    // what capture_end hands to the graph
    struct Snapshot {
        uint32_t slots = 0;                                     // bit s: the capture reserved slot s
        uint64_t slot_gen[SLOTS] = {0, 0, 0, 0, 0};
        std::vector<std::pair<uint64_t, uint64_t>> plans;       // (serial, generation) of every plan the capture called
    };

    uint64_t slot_gen[SLOTS] = {0, 0, 0, 0, 0};
    uint64_t next_serial = 1;                   // serials are 1, 2, 3, ...; 0 = "no plan"
    std::map<uint64_t, uint64_t> plan_gen;      // the live plans
    bool capturing = false;
    uint32_t noted_slots = 0;
    std::vector<uint64_t> noted_plans;          // serials, each once, in the order of their first call

    uint64_t plan_created() {
        const uint64_t s = next_serial++;
        plan_gen[s] = 0;
        return s;
    }
    void plan_buffer_reallocated(uint64_t serial) {
        auto it = plan_gen.find(serial);
        if (it != plan_gen.end()) it->second++;
    }
    void plan_destroyed(uint64_t serial) { plan_gen.erase(serial); }
    void slot_reallocated(int slot) {
        if (slot >= 0 && slot < SLOTS) slot_gen[slot]++;
    }

    void capture_begin() {
        capturing = true;
        noted_slots = 0;
        noted_plans.clear();
    }
    void slot_used(int slot) {
        if (capturing && slot >= 0 && slot < SLOTS) noted_slots |= 1u << slot;
    }
    void plan_used(uint64_t serial) {
        if (!capturing || !serial) return;
        for (uint64_t s : noted_plans)
            if (s == serial) return;
        noted_plans.push_back(serial);
    }
    Snapshot capture_end() {
        Snapshot S;
        S.slots = noted_slots;
        for (int i = 0; i < SLOTS; i++) S.slot_gen[i] = slot_gen[i];
        for (uint64_t s : noted_plans) {
            auto it = plan_gen.find(s);
            // (a plan cannot be destroyed while its context captures -- j2k_plan_destroy synchronises; were it gone all the same, a generation
            // no live plan has at its creation keeps the graph stale for good: verdict() finds no entry)
            S.plans.emplace_back(s, it != plan_gen.end() ? it->second : 0);
        }
        capturing = false;
        noted_slots = 0;
        noted_plans.clear();
        return S;
    }

    // which: the slot (a) or the plan's serial (b, c) the verdict is about
    Verdict verdict(const Snapshot &S, uint64_t *which = nullptr) const {
        for (int i = 0; i < SLOTS; i++)
            if ((S.slots >> i & 1u) && S.slot_gen[i] != slot_gen[i]) {
                if (which) *which = (uint64_t)i;
                return STALE_SLOT;
            }
        Verdict v = VALID;
        for (const auto &p : S.plans) {
            auto it = plan_gen.find(p.first);
            if (it == plan_gen.end()) {          // (c) outranks (b): the plan's every buffer is gone
                if (which) *which = p.first;
                return STALE_PLAN_DESTROYED;
            }
            if (it->second != p.second && v == VALID) {
                if (which) *which = p.first;
                v = STALE_PLAN_BUFFER;
            }
        }
        return v;
    }
};

}  // namespace j2k

// graph_guard_main.cpp -- CPU: the graph lifetime bookkeeping (go-jpeg2000_amd/csrc/graph_guard.h) driven through scripted histories; one line
// per verdict, "<history>.<check> <verdict>[:<slot or serial>]".  tests/test_graph_guard.py holds the expected table, written out by hand,
// and builds this file plain and with AddressSanitizer + UBSan.  The histories are the calls the library makes: capture_begin, slot_used from
// stage_reserve, plan_used from the plan entry points, capture_end, then slot_reallocated / plan_buffer_reallocated / plan_destroyed.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../go-jpeg2000_amd/csrc/graph_guard.h"

using j2k::GraphGuard;

static const char *kName[] = {"valid", "stale_a", "stale_b", "stale_c"};

static void say(const char *what, const GraphGuard &G, const GraphGuard::Snapshot &S) {
    uint64_t which = 0;
    const GraphGuard::Verdict v = G.verdict(S, &which);
    if (v == GraphGuard::VALID) printf("%s %s\n", what, kName[v]);
    else printf("%s %s:%llu\n", what, kName[v], (unsigned long long)which);
}
static GraphGuard::Snapshot capture(GraphGuard &G, std::initializer_list<int> slots, std::initializer_list<uint64_t> plans) {
    G.capture_begin();
    for (int s : slots) G.slot_used(s);
    for (uint64_t p : plans) G.plan_used(p);
    return G.capture_end();
}

int main() {
    {   // slots: a capture that used {0, 2}
        GraphGuard G;
        const uint64_t A = G.plan_created();
        const GraphGuard::Snapshot S = capture(G, {0, 2, 0}, {A});
        printf("slots.noted %u\n", S.slots);                       // reserved with no growth = noted as used
        say("slots.fresh", G, S);
        G.slot_reallocated(1);
        say("slots.grow1", G, S);
        G.slot_reallocated(3); G.slot_reallocated(4);
        say("slots.grow34", G, S);
        G.slot_reallocated(2);
        say("slots.grow2", G, S);
        G.slot_reallocated(0);
        say("slots.grow0", G, S);                                  // the lowest stale slot is named
    }
    {   // outside a capture nothing is noted, and a capture starts from nothing
        GraphGuard G;
        const uint64_t A = G.plan_created();
        G.slot_used(1); G.plan_used(A);
        const GraphGuard::Snapshot S = capture(G, {3}, {});
        printf("idle.noted %u %zu\n", S.slots, S.plans.size());
        G.slot_reallocated(1); G.plan_buffer_reallocated(A); G.plan_destroyed(A);
        say("idle.after", G, S);
        const GraphGuard::Snapshot S2 = capture(G, {}, {});        // the notes of the capture before do not leak into the next
        printf("idle.second %u %zu\n", S2.slots, S2.plans.size());
    }
    {   // two plans, a graph each; then B grows its buffer, then A is destroyed, then a new plan "at A's address"
        GraphGuard G;
        const uint64_t A = G.plan_created(), B = G.plan_created();
        printf("plans.serials %llu %llu\n", (unsigned long long)A, (unsigned long long)B);
        const GraphGuard::Snapshot SA = capture(G, {0}, {A, A}), SB = capture(G, {0}, {B});
        printf("plans.noted %zu %zu\n", SA.plans.size(), SB.plans.size());
        say("plans.A0", G, SA); say("plans.B0", G, SB);
        G.plan_buffer_reallocated(B);
        say("plans.A1", G, SA); say("plans.B1", G, SB);
        G.plan_destroyed(A);
        say("plans.A2", G, SA); say("plans.B2", G, SB);
        const uint64_t A2 = G.plan_created();                      // the allocator may hand it A's addresses: the serial is new
        printf("plans.reborn %llu\n", (unsigned long long)A2);
        say("plans.A3", G, SA);
        const GraphGuard::Snapshot SA2 = capture(G, {0}, {A2});
        say("plans.A2graph", G, SA2); say("plans.A4", G, SA);
        // stale, then captured again: the new graph is valid, the old one stays stale
        const GraphGuard::Snapshot SB2 = capture(G, {0}, {B});
        say("plans.Bnew", G, SB2); say("plans.Bold", G, SB);
        // a graph over both plans: (c) outranks (b) whatever the order of the calls
        const GraphGuard::Snapshot SX = capture(G, {}, {B, A2});
        G.plan_buffer_reallocated(B);
        say("plans.X1", G, SX);
        G.plan_destroyed(A2);
        say("plans.X2", G, SX);
        say("plans.Bnew2", G, SB2);
        // growth and destruction of an unknown serial (a plan of another context never reaches this table) change nothing
        const GraphGuard::Snapshot SB3 = capture(G, {}, {B});
        G.plan_buffer_reallocated(99); G.plan_destroyed(99); G.plan_destroyed(A);
        say("plans.Bnewest", G, SB3);
        say("plans.A2graph2", G, SA2);
    }
    {   // slot growth and plan growth together: (a) is reported first
        GraphGuard G;
        const uint64_t A = G.plan_created();
        const GraphGuard::Snapshot S = capture(G, {4}, {A});
        G.plan_buffer_reallocated(A); G.slot_reallocated(4);
        say("both.ab", G, S);
    }
    {   // wrap: the counters are uint64_t and compared for equality.  From a snapshot taken at the top of the range, 2^k further bumps
        // (k = 0 ... 63, set directly: the compare is what is tested) never read as valid; only 2^64 = 0 more would
        GraphGuard G;
        const uint64_t A = G.plan_created();
        G.slot_gen[2] = UINT64_MAX; G.plan_gen[A] = UINT64_MAX;
        const GraphGuard::Snapshot S = capture(G, {2}, {A});
        say("wrap.fresh", G, S);
        G.slot_reallocated(2); G.plan_buffer_reallocated(A);       // both wrap to 0
        printf("wrap.gens %llu %llu\n", (unsigned long long)G.slot_gen[2], (unsigned long long)G.plan_gen[A]);
        say("wrap.one", G, S);
        int stale_a = 0, stale_b = 0;
        for (int k = 0; k < 64; k++) {
            G.slot_gen[2] = S.slot_gen[2] + (uint64_t(1) << k);
            stale_a += G.verdict(S) == GraphGuard::STALE_SLOT;
        }
        G.slot_gen[2] = S.slot_gen[2];
        for (int k = 0; k < 64; k++) {
            G.plan_gen[A] = S.plans[0].second + (uint64_t(1) << k);
            stale_b += G.verdict(S) == GraphGuard::STALE_PLAN_BUFFER;
        }
        printf("wrap.pow2 %d %d\n", stale_a, stale_b);
        G.plan_gen[A] = S.plans[0].second;
        say("wrap.back", G, S);                                    // exactly 2^64 bumps of each: the one history that reads valid again
        printf("wrap.width %zu %zu\n", sizeof(G.slot_gen[0]) * 8, sizeof(G.next_serial) * 8);
    }
    return 0;
}

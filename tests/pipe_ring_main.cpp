// pipe_ring_main.cpp -- drives csrc/pipe_ring.h (the bookkeeping of the pipelined host codec) on the CPU with a scripted event oracle, under
// AddressSanitizer + UBSan (tests/test_pipe_ring.py builds and runs it).  The oracle is the D2H copy stream as a FIFO of operations
// ("small copy of ticket t", "payload copy of ticket t"): an operation is done once popped, a blocking wait pops up to it, a "complete" step pops
// one.  Against that model, over seeded interleavings of submit / complete / poll / wait at every depth:
//   - tickets are 1, 2, 3, ...; a submit beyond `depth` un-waited tickets gets no slot and consumes no ticket (the un-waited limit);
//   - a payload copy is queued once per frame, in ticket order, and never before the frame's small copy (its length) has arrived;
//   - a small copy is queued once per frame, in ticket order, and never before the payload copy of every older frame was queued (the stream's
//     order is small(1), payload(1), small(2), ...: no payload copy waits behind a younger frame's kernels);
//   - no slot is taken again before both copies of the frame that had it completed;
//   - a waited ticket is gone (find), a ticket never issued is unknown, retire is refused before the payload stage or without its copy done.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <random>
#include <set>

#include "../go-jpeg2000_amd/csrc/pipe_ring.h"

using j2k::PipeRing;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "%s:%d: CHECK(%s) failed (depth %d, seed %u, step %d)\n", __FILE__, __LINE__, #cond, g_depth, g_seed, g_step); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

static int g_depth = 0, g_step = 0;
static unsigned g_seed = 0;

struct Op { bool payload; uint64_t ticket; };
struct Model {
    std::deque<Op> fifo;                       // the copy stream: queued, not yet done
    std::set<uint64_t> small_done, pay_done, small_queued, pay_queued, unwaited;
    std::map<int, uint64_t> slot_ticket;       // the ticket that last had a slot
    uint64_t issued = 0, last_pay_queued = 0;
    void pop() {
        const Op o = fifo.front();
        fifo.pop_front();
        (o.payload ? pay_done : small_done).insert(o.ticket);
    }
    void pop_until(bool payload, uint64_t ticket) {
        while (!(payload ? pay_done : small_done).count(ticket)) {
            if (fifo.empty()) { fprintf(stderr, "model: waiting for an operation that was never queued\n"); exit(1); }
            pop();
        }
    }
};

static long run(int depth, unsigned seed, int steps) {
    g_depth = depth; g_seed = seed;
    std::mt19937 rng(seed * 9176u + (unsigned)depth);
    PipeRing ring;
    CHECK(ring.init(depth));
    Model m;
    long waits = 0;
    auto queue_small = [&](int s) {
        const uint64_t t = ring.slots[s].ticket;
        CHECK(ring.slots[s].state == PipeRing::KERNELS);
        CHECK(!m.small_queued.count(t));                    // once
        CHECK(m.last_pay_queued == t - 1);                  // behind the payload copy of every older frame, and in ticket order
        m.small_queued.insert(t);
        m.fifo.push_back(Op{false, t});
    };
    auto small_done = [&](int s, bool block) {
        const uint64_t t = ring.slots[s].ticket;
        CHECK(ring.slots[s].state == PipeRing::SMALL && m.small_queued.count(t));
        if (block) m.pop_until(false, t);
        return m.small_done.count(t) != 0;
    };
    auto queue_payload = [&](int s) {
        const uint64_t t = ring.slots[s].ticket;
        CHECK(m.small_done.count(t));                       // never before its length arrived
        CHECK(!m.pay_queued.count(t));                      // once
        CHECK(t == m.last_pay_queued + 1);                  // in ticket order, none left out
        m.last_pay_queued = t;
        m.pay_queued.insert(t);
        m.fifo.push_back(Op{true, t});
    };
    for (g_step = 0; g_step < steps; g_step++) {
        const unsigned a = rng() % 100;
        if (a < 35) {                                       // submit
            const int s = ring.free_slot();
            CHECK((s < 0) == ((int)m.unwaited.size() == depth));
            CHECK(ring.unwaited() == (int)m.unwaited.size());
            if (s < 0) { CHECK(ring.next_ticket == m.issued + 1); continue; }
            ring.pump(0, queue_small, small_done, queue_payload);        // (as a submit does)
            CHECK(ring.slots[s].state == PipeRing::FREE);
            if (m.slot_ticket.count(s)) {                   // the frame that had this slot: both copies done, and waited
                const uint64_t old = m.slot_ticket[s];
                CHECK(m.small_done.count(old) && m.pay_done.count(old) && !m.unwaited.count(old));
            }
            const uint64_t t = ring.commit(s);
            CHECK(t == ++m.issued);
            m.slot_ticket[s] = t;
            m.unwaited.insert(t);
            CHECK(ring.find(t) == s);
            ring.pump(0, queue_small, small_done, queue_payload);                          // (as a submit does, behind its kernels)
            CHECK(m.small_queued.count(t) == (m.last_pay_queued + 1 >= t ? 1u : 0u));
        } else if (a < 60) {                                // the device completes one operation
            if (!m.fifo.empty()) m.pop();
        } else if (a < 75) {                                // poll of a random un-waited ticket
            if (m.unwaited.empty()) continue;
            auto it = m.unwaited.begin();
            std::advance(it, rng() % m.unwaited.size());
            const int s = ring.find(*it);
            CHECK(s >= 0);
            ring.pump(0, queue_small, small_done, queue_payload);
            const bool done = ring.payload_queued(s) && m.pay_done.count(*it);
            if (done) CHECK(m.small_done.count(*it));
        } else if (a < 95) {                                // wait of a random un-waited ticket (any order)
            if (m.unwaited.empty()) continue;
            auto it = m.unwaited.begin();
            std::advance(it, rng() % m.unwaited.size());
            const uint64_t t = *it;
            const int s = ring.find(t);
            CHECK(s >= 0 && ring.slots[s].ticket == t);
            if (ring.slots[s].state != PipeRing::PAYLOAD) CHECK(!ring.retire(s, true));    // not before the payload stage
            ring.pump(t, queue_small, small_done, queue_payload);
            CHECK(ring.payload_queued(s) && m.pay_queued.count(t));
            for (uint64_t e : m.unwaited) if (e < t) CHECK(m.pay_queued.count(e));          // earlier frames' copies were queued first
            CHECK(!ring.retire(s, false));                  // not without its copy done
            CHECK(ring.find(t) == s);
            m.pop_until(true, t);
            CHECK(ring.retire(s, true));
            m.unwaited.erase(t);
            CHECK(ring.find(t) < 0);                        // waited: gone
            CHECK(ring.slots[s].state == PipeRing::FREE);
            waits++;
        } else {                                            // stale and unknown tickets
            CHECK(ring.find(0) < 0);
            CHECK(ring.find(m.issued + 1) < 0 && ring.find(m.issued + 1 + rng() % 1000) < 0);
            if (m.issued) {
                const uint64_t t = 1 + rng() % m.issued;
                CHECK((ring.find(t) >= 0) == (m.unwaited.count(t) != 0));
            }
        }
    }
    // drain: everything queued, every ticket still waitable
    ring.pump(~uint64_t(0), queue_small, small_done, queue_payload);
    for (uint64_t t : m.unwaited) {
        const int s = ring.find(t);
        CHECK(s >= 0 && ring.payload_queued(s));
        m.pop_until(true, t);
        CHECK(ring.retire(s, true));
        waits++;
    }
    CHECK(ring.unwaited() == 0 && ring.free_slot() >= 0);
    CHECK(m.last_pay_queued == m.issued && m.pay_done.size() == m.issued && m.small_queued.size() == m.issued);
    return waits;
}

int main(int argc, char **argv) {
    const int seeds = argc > 1 ? atoi(argv[1]) : 64, steps = argc > 2 ? atoi(argv[2]) : 400;
    PipeRing bad;
    if (bad.init(0) || bad.init(9) || bad.init(-1)) { fprintf(stderr, "init accepted a depth outside 1 ... 8\n"); return 1; }
    long waits = 0, runs = 0;
    for (int depth = 1; depth <= PipeRing::MAX_DEPTH; depth++)
        for (int seed = 0; seed < seeds; seed++) { waits += run(depth, (unsigned)seed, steps); runs++; }
    printf("pipe_ring ok: %ld interleavings, %ld waits\n", runs, waits);
    return 0;
}

// pipe_ring.h -- the bookkeeping of the pipelined host codec (j2k_pipe.cpp), without any HIP in it: ticket -> slot, the slot states, which copy
// may be queued when, the un-waited limit.  Its callers inject the "is this event done" answers, so tests/pipe_ring_main.cpp drives it on the
// CPU with a scripted event oracle.
//
// A frame's life.  FREE -> (submit: the H2D copy and the kernels are queued) KERNELS -> (pump: the small copy back -- status, length, tables --
// is queued) SMALL -> (pump: the small copy has arrived, so the payload copy was queued at its exact length, or found unnecessary) PAYLOAD ->
// (wait: the payload copy has arrived, the results were handed over) FREE.
//
// The order on the one D2H stream is small(1), payload(1), small(2), payload(2), ...: a frame's small copy is queued only once the payload
// copy of the frame before it has been queued.  A small copy waits for its frame's kernels; queued early it would sit at the head of the
// stream in front of the earlier frame's payload copy, and that copy -- and the wait that returns the slot to the next submit -- would wait
// for kernels it has nothing to do with: copies and kernels would take turns.  So at most one frame is in SMALL, every older un-waited frame
// is in PAYLOAD, every younger one in KERNELS.  A slot is taken again only after its ticket was waited, i.e. after both of its copies completed.
#pragma once
#include <cstdint>

namespace j2k {

struct PipeRing {
    static constexpr int MAX_DEPTH = 8;
    enum State { FREE = 0, KERNELS = 1, SMALL = 2, PAYLOAD = 3 };
    struct Slot { int state = FREE; uint64_t ticket = 0; };
    int depth = 0;
    uint64_t next_ticket = 1;          // tickets are 1, 2, 3, ...: a refused submit consumes none
    Slot slots[MAX_DEPTH];

    bool init(int d) {
        if (d < 1 || d > MAX_DEPTH) return false;
        depth = d;
        next_ticket = 1;
        for (Slot &s : slots) s = Slot();
        return true;
    }
    int unwaited() const {
        int n = 0;
        for (int i = 0; i < depth; i++) n += slots[i].state != FREE;
        return n;
    }
    // the slot a submit may fill, or -1: `depth` tickets are un-waited.  Nothing changes until commit().
    int free_slot() const {
        for (int i = 0; i < depth; i++)
            if (slots[i].state == FREE) return i;
        return -1;
    }
    // the submit queued its kernels on `slot` (from free_slot()): the frame's ticket
    uint64_t commit(int slot) {
        slots[slot].state = KERNELS;
        slots[slot].ticket = next_ticket;
        return next_ticket++;
    }
    // the slot of an un-waited ticket, or -1 (unknown, or waited before)
    int find(uint64_t ticket) const {
        if (ticket == 0 || ticket >= next_ticket) return -1;
        for (int i = 0; i < depth; i++)
            if (slots[i].state != FREE && slots[i].ticket == ticket) return i;
        return -1;
    }
    // the slot with the lowest ticket whose payload stage is still ahead (KERNELS or SMALL), or -1
    int oldest_pending() const {
        int best = -1;
        for (int i = 0; i < depth; i++)
            if ((slots[i].state == KERNELS || slots[i].state == SMALL) && (best < 0 || slots[i].ticket < slots[best].ticket)) best = i;
        return best;
    }
    // Queue the copies that may be queued, in ticket order.  queue_small(slot): once per frame, when every older frame's payload copy has been
    // queued.  small_done(slot, block): has the slot's small copy arrived -- with block set the caller waits for it and answers true; frames
    // up to ticket `upto` are waited for (0: none, ~0: all), later ones only asked.  queue_payload(slot): once per frame, after its small copy
    // arrived and never before.
    template <typename QueueSmall, typename SmallDone, typename QueuePayload>
    void pump(uint64_t upto, QueueSmall queue_small, SmallDone small_done, QueuePayload queue_payload) {
        for (;;) {
            const int s = oldest_pending();
            if (s < 0) return;
            if (slots[s].state == KERNELS) {
                queue_small(s);
                slots[s].state = SMALL;
            }
            if (!small_done(s, slots[s].ticket <= upto)) return;
            queue_payload(s);
            slots[s].state = PAYLOAD;
        }
    }
    bool payload_queued(int slot) const { return slots[slot].state == PAYLOAD; }
    // the ticket was waited: its slot is free again.  Refused (false) unless the payload stage was reached and the caller saw its copy done.
    bool retire(int slot, bool payload_done) {
        if (slots[slot].state != PAYLOAD || !payload_done) return false;
        slots[slot].state = FREE;
        return true;
    }
};

}  // namespace j2k

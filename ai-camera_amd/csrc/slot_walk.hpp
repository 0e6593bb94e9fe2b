// slot_walk.hpp -- the life cycle of a per-stream table of 512 track slots on the device, once: what the best-shot and the colour walk
// kernels share (device code only; included by kernels_bestshot.hip and kernels_colours.hip).
//
// ONE block of 512 threads walks the launch's ticks of one stream in order (blockIdx.x = stream): a thread is slot t of the table AND row t
// of the frame.  The table's small arrays live in LDS for the launch.  A launch:
//   load the table, or zero it on a pending reset -> without ticks: drain or flush as mode[stream] says -> per tick: the row's info and
//   whether it is counted (VALID, FIRST of its id, NONEMPTY); the slot's expiry by forget_after; the id lookup among the live slots; five
//   block scans; the capacity rule (the tick's live + ENDED that stay + new rows exceed max_tracks: the stream stops with
//   AIC_ERR_CAPACITY and NOTHING of this tick is committed); ENDED slots leave for the output list in slot order while it has room and
//   become free; the k-th new row takes the k-th lowest free slot; counted rows commit -> frame, stopped and the table written back,
//   n_final, pending and status of the stream.
//
// slot_walk<V> is instantiated with a variant V, an object of the kernel that holds the variant's own arguments and LDS arrays and states,
// as __forceinline__ members, what its stage does differently:
//   ARRAYS, ST_INTS, EVENT_INTS       the table's arrays (the first SLOT_A_SHARED are the skeleton's), a stream's state, an event
//   Row, load_row                     what a thread keeps of its row: flags, and the info of its own
//   fresh                             the initial values of a new slot's own arrays
//   commit                            a counted row's own part, behind the skeleton's (last_seen, cls, sightings)
//   event                             the event of an ENDED slot that leaves (slot_event_head writes the shared eight ints' first seven)
//   post_emit                         behind the events: the variant's barriers, its copies, and the slot set free between them
//   post_tick                         behind the commits: what the tick delivers (thumbnails to their slots; row tags)
//   tail                              behind the last tick: what is owed for the ticks a stopped stream did not walk
// The barriers inside post_emit and post_tick are the variant's: they order its reads of a slot's data before a row may take the slot.
// The skeleton never asks which variant it runs.
#pragma once
#include "bank_call.hpp"
#include "stage_dev.hpp"

namespace aic {
namespace {

// the launch arguments that every slot stage has
struct SlotCall {
    const int* frame_off;
    int n_ticks;
    const int* rows6;
    const int* reset;
    const int* mode;
    int first, streams, max_tracks, forget_after;
    int* state_all;
    int cap;
    int *n_final, *pending, *status, *events;
};

// the block's LDS as the hooks see it: the table, and the skeleton's lists (free between the skeleton's uses: see slot_walk)
struct SlotLds {
    int (*tab)[SLOT_TRACKS];
    int *live, *list, *w;
};

// ints 0..6 of an event, and the variant's eighth
__device__ __forceinline__ void slot_event_head(const SlotLds& L, int4* ev, int s, int w7) {
    const int tid = threadIdx.x;
    ev[0] = make_int4(L.tab[SLOT_A_STATE][tid] == 3 ? SLOT_FLUSHED : SLOT_EXPIRED, s, L.tab[SLOT_A_ID][tid], L.tab[SLOT_A_CLS][tid]);
    ev[1] = make_int4(L.tab[SLOT_A_FIRST][tid], L.tab[SLOT_A_LAST][tid], L.tab[SLOT_A_SIGHT][tid], w7);
}

template <class V>
__device__ __forceinline__ void slot_walk(const SlotCall& c, V& v) {
    constexpr int T = SLOT_TRACKS;
    __shared__ int s_tab[V::ARRAYS][T];
    __shared__ int s_live[T], s_list[T];
    __shared__ int s_w[8];
    const SlotLds L{s_tab, s_live, s_list, s_w};
    int* s_id = s_tab[SLOT_A_ID];
    int* s_state = s_tab[SLOT_A_STATE];
    int* s_last = s_tab[SLOT_A_LAST];
    const int s = blockIdx.x, tid = threadIdx.x, S = c.streams, cap = c.cap;
    int* st = c.state_all + (size_t)s * V::ST_INTS;
    const bool fresh = c.first && c.reset[s];
    int frame = fresh ? 0 : st[0];
    int stopped = fresh ? 0 : st[1];
#pragma unroll
    for (int a = 0; a < V::ARRAYS; ++a) s_tab[a][tid] = fresh ? 0 : st[SLOT_ST_SLOTS + a * T + tid];
    int n_out = c.first ? 0 : c.n_final[s];
    __syncthreads();

    // ENDED slots (E, ranked e_rank in slot order) leave for the output list while it has room; they become free
    auto emit = [&](bool E, int e_rank, int n_E) {
        const int room = cap - n_out;
        const bool em = E && e_rank < room;
        if (em) v.event(L, reinterpret_cast<int4*>(c.events + ((size_t)s * cap + n_out + e_rank) * V::EVENT_INTS), s, e_rank);
        const int n_emit = n_E < room ? n_E : (room > 0 ? room : 0);
        v.post_emit(L, em, n_emit, n_out);
        n_out += n_emit;
    };

    if (c.n_ticks == 0) {
        const int m = c.mode[s];
        if (m == SLOT_MODE_FLUSH && s_state[tid] == 1) s_state[tid] = 3;
        if (m != SLOT_MODE_NONE) {
            const bool E = tid < c.max_tracks && s_state[tid] >= 2;
            int n_E;
            const int e_rank = block_scan(E, s_w, n_E);
            emit(E, e_rank, n_E);
        }
    }
    int kk = 0;
    for (; kk < c.n_ticks && !stopped; ++kk) {
        const int x = kk * S + s;
        const int off = c.frame_off[x], n = c.frame_off[x + 1] - off;        // 0..512, checked by the host
        // ---- this thread as row tid
        typename V::Row row = v.load_row(off + tid, tid < n);
        int rid = 0, rcls = 0;
        if (tid < n) rid = c.rows6[(size_t)(off + tid) * 6 + 4], rcls = c.rows6[(size_t)(off + tid) * 6 + 5];
        const int need = SLOT_F_VALID | SLOT_F_FIRST | SLOT_F_NONEMPTY;
        const bool counted = (row.flags & need) == need;
        // ---- this thread as slot tid
        const int state = tid < c.max_tracks ? s_state[tid] : 0;
        const bool expiring = state == 1 && frame - s_last[tid] > c.forget_after;
        const bool E = state >= 2 || expiring;
        s_live[tid] = state == 1 && !expiring;
        __syncthreads();
        int slot = -1;
        if (counted)
            for (int t = 0; t < c.max_tracks; ++t)
                if (s_live[t] && s_id[t] == rid) slot = t;
        const bool is_new = counted && slot < 0;
        int n_new, n_E, n_live, n_old, n_unfit;
        const int new_rank = block_scan(is_new, s_w, n_new);
        const int e_rank = block_scan(E, s_w, n_E);
        block_scan(s_live[tid], s_w, n_live);
        block_scan(state >= 2, s_w, n_old);
        block_scan(expiring && e_rank >= cap - n_out, s_w, n_unfit);         // ENDED now, no room in the list: the slot stays taken
        if (n_live + n_old + n_unfit + n_new > c.max_tracks) {               // nothing of this tick is committed
            stopped = AIC_ERR_CAPACITY;
            break;
        }
        if (expiring) s_state[tid] = 2;
        emit(E, e_rank, n_E);
        const bool is_free = tid < c.max_tracks && s_state[tid] == 0;
        int n_free;
        const int free_rank = block_scan(is_free, s_w, n_free);
        if (is_free) s_list[free_rank] = tid;
        __syncthreads();
        if (counted) {
            const bool fresh_slot = slot < 0;
            if (fresh_slot) {                                                // the k-th new row takes the k-th lowest free slot
                slot = s_list[new_rank];
                s_id[slot] = rid, s_state[slot] = 1, s_tab[SLOT_A_FIRST][slot] = frame, s_tab[SLOT_A_SIGHT][slot] = 0;
                v.fresh(L, slot);
            }
            s_last[slot] = frame, s_tab[SLOT_A_CLS][slot] = rcls, s_tab[SLOT_A_SIGHT][slot] += 1;
            v.commit(L, row, slot, fresh_slot, frame);
        }
        v.post_tick(L, row, slot, off, n, stopped);
        ++frame;
        __syncthreads();
    }
    __syncthreads();
    v.tail(c, kk);
#pragma unroll
    for (int a = 0; a < V::ARRAYS; ++a) st[SLOT_ST_SLOTS + a * T + tid] = s_tab[a][tid];
    int n_pend;
    block_scan(tid < c.max_tracks && s_state[tid] >= 2, s_w, n_pend);
    if (tid == 0) st[0] = frame, st[1] = stopped, c.n_final[s] = n_out, c.pending[s] = n_pend, c.status[s] = stopped;
}

}  // namespace
}  // namespace aic

// The optional outputs a caller binds for ONE batch call -- consensus codes (skx_stream_bind_consensus), the change list
// (skx_stream_bind_changes), the species call and its own change list (skx_stream_bind_call, skx_stream_bind_call_changes) -- as one
// record.  The same record holds the caller's arrays (skx_stream::bound), a holder's device arrays (host-fed batches) and what the
// kernels of a PendingBatch / SubPass write.  Plain C++ (no HIP): tests/test_batch_out_cpu.py compiles this header alone.
#pragma once
#include <stddef.h>

namespace skx {

// An event list: the reads at which the call changes, compacted.  cap == 0: none.  ev_sp exists only for the species call's list
// (NULL for the plain change list); a list with ev_codes compares the codes of two reads, one without their index rows.
struct EventList {
    unsigned cap = 0;
    unsigned n_batch = 0;  // reads of the batch: the sub-pass that ends there queues the scan and the gathers
    unsigned *n_events = nullptr, *ev_read = nullptr, *ev_sp = nullptr, *ev_idx = nullptr;
    unsigned long long* ev_sum = nullptr;
    unsigned* ev_codes = nullptr;
    bool codes() const { return ev_codes != nullptr; }
};
// Compact rows of the species call, one per read.  on: bound (sp is then mandatory).
struct CallRows {
    bool on = false;
    unsigned *sp = nullptr, *idx = nullptr;
    unsigned long long* sum = nullptr;
    unsigned* codes = nullptr;
};
struct BatchOut {
    unsigned* cons = nullptr;  // [n_reads][n_species][n_features]; in a device record: where the batch's votes go (NULL: the ranking lane's scratch)
    EventList chg;
    CallRows call;
    EventList call_ev;
    bool any() const { return cons || chg.cap || wants_call(); }
    bool wants_call() const { return call.on || call_ev.cap != 0; }
    // somebody reads the consensus codes of the batch's rows
    bool wants_vote() const { return cons || chg.codes() || call.codes || call_ev.codes(); }
    void set_batch(unsigned n_reads) { chg.n_batch = call_ev.n_batch = n_reads; }
};

// Words per entry of an event list's (and per read of the call rows') index / sum and codes columns.
struct RowWidths { size_t idx, codes; };
inline RowWidths change_widths(unsigned n_species, unsigned top_k, unsigned n_features) {
    return RowWidths{(size_t)n_species * top_k, (size_t)n_species * n_features};
}
inline RowWidths call_widths(unsigned top_k, unsigned n_features) { return RowWidths{top_k, n_features}; }

// What the kernels get: the device arrays `have` for the columns the caller asked for in `want` (and the mandatory ones); an unbound
// `want` gives an all-NULL record.
inline EventList device_view(const EventList& want, const EventList& have) {
    EventList c;
    if (want.cap == 0) return c;
    c.cap = want.cap < have.cap ? want.cap : have.cap;
    c.n_events = have.n_events; c.ev_read = have.ev_read;
    c.ev_sp = want.ev_sp ? have.ev_sp : nullptr;
    c.ev_idx = want.ev_idx ? have.ev_idx : nullptr;
    c.ev_sum = want.ev_sum ? have.ev_sum : nullptr;
    c.ev_codes = want.ev_codes ? have.ev_codes : nullptr;
    return c;
}
inline CallRows device_view(const CallRows& want, const CallRows& have) {
    CallRows c;
    if (!want.on) return c;
    c.on = true;
    c.sp = have.sp;
    c.idx = want.idx ? have.idx : nullptr;
    c.sum = want.sum ? have.sum : nullptr;
    c.codes = want.codes ? have.codes : nullptr;
    return c;
}
inline BatchOut device_view(const BatchOut& want, const BatchOut& have) {
    BatchOut c;
    c.cons = want.wants_vote() ? have.cons : nullptr;
    c.chg = device_view(want.chg, have.chg);
    c.call = device_view(want.call, have.call);
    c.call_ev = device_view(want.call_ev, have.call_ev);
    return c;
}

}  // namespace skx

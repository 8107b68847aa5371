// Stand-alone check of sketchy_amd/csrc/skx_batch_out.hpp (plain C++, no HIP): the record of a batch's bound outputs and the view of
// a holder's device arrays the kernels get for it.  Every combination of bound optional columns, for both kinds of event list, the
// call rows and the whole record, against fake device arrays: the view hands a device pointer for exactly the columns asked for plus
// the mandatory ones, cap is min(want, have), an unbound record gives an all-NULL view, and wants_vote() is true exactly when somebody
// reads codes.  Built and run by tests/test_batch_out_cpu.py (with -fsanitize=address,undefined).  Prints "<checks> checks, <n> failures".
#include <stdio.h>

#include "skx_batch_out.hpp"

static long n_checks = 0, n_fail = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        ++n_checks;                                                              \
        if (!(c)) { ++n_fail; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

using skx::BatchOut;
using skx::CallRows;
using skx::EventList;

// the caller's arrays and the "device" arrays: distinct objects, never dereferenced
static unsigned host_w[16], dev_w[16];
static unsigned long long host_l[4], dev_l[4];

// an event list over the arrays w[base ..] / l[base_l]; bits: 1 idx, 2 sum, 4 codes; all: every column (a holder's arrays)
static EventList make_events(unsigned* w, unsigned long long* l, unsigned base, unsigned base_l, unsigned cap, unsigned bits, bool species) {
    EventList e;
    e.cap = cap;
    e.n_events = w + base; e.ev_read = w + base + 1;
    if (species) e.ev_sp = w + base + 2;
    if (bits & 1u) e.ev_idx = w + base + 3;
    if (bits & 2u) e.ev_sum = l + base_l;
    if (bits & 4u) e.ev_codes = w + base + 4;
    return e;
}
static CallRows make_rows(unsigned* w, unsigned long long* l, unsigned bits) {
    CallRows c;
    c.on = true;
    c.sp = w + 10;
    if (bits & 1u) c.idx = w + 11;
    if (bits & 2u) c.sum = l + 2;
    if (bits & 4u) c.codes = w + 12;
    return c;
}
static bool all_null(const EventList& e) {
    return e.cap == 0 && e.n_batch == 0 && !e.n_events && !e.ev_read && !e.ev_sp && !e.ev_idx && !e.ev_sum && !e.ev_codes && !e.codes();
}
static bool all_null(const CallRows& c) { return !c.on && !c.sp && !c.idx && !c.sum && !c.codes; }

static void check_events_view(const EventList& want, const EventList& have, const EventList& v, unsigned bits, bool species) {
    CHECK(v.cap == (want.cap < have.cap ? want.cap : have.cap));
    CHECK(v.n_events == have.n_events && v.ev_read == have.ev_read);  // mandatory
    CHECK(v.ev_sp == (species ? have.ev_sp : nullptr));
    CHECK(v.ev_idx == ((bits & 1u) ? have.ev_idx : nullptr));
    CHECK(v.ev_sum == ((bits & 2u) ? have.ev_sum : nullptr));
    CHECK(v.ev_codes == ((bits & 4u) ? have.ev_codes : nullptr));
    CHECK(v.codes() == ((bits & 4u) != 0));
    CHECK(v.n_batch == 0);
}
static void check_rows_view(const CallRows& have, const CallRows& v, unsigned bits) {
    CHECK(v.on && v.sp == have.sp);  // mandatory
    CHECK(v.idx == ((bits & 1u) ? have.idx : nullptr));
    CHECK(v.sum == ((bits & 2u) ? have.sum : nullptr));
    CHECK(v.codes == ((bits & 4u) ? have.codes : nullptr));
}

int main() {
    const unsigned caps[] = {1u, 5u, 9u};
    // ---- the two kinds of list alone: every set of optional columns, caps below, at and above the holder's
    for (int species = 0; species < 2; ++species) {
        const EventList have = make_events(dev_w, dev_l, species ? 5u : 0u, species ? 1u : 0u, 5u, 7u, species != 0);
        for (unsigned bits = 0; bits < 8; ++bits)
            for (unsigned cap : caps) {
                const EventList want = make_events(host_w, host_l, species ? 5u : 0u, species ? 1u : 0u, cap, bits, species != 0);
                check_events_view(want, have, skx::device_view(want, have), bits, species != 0);
            }
        CHECK(all_null(skx::device_view(EventList{}, have)));
    }
    {
        const CallRows have = make_rows(dev_w, dev_l, 7u);
        for (unsigned bits = 0; bits < 8; ++bits) check_rows_view(have, skx::device_view(make_rows(host_w, host_l, bits), have), bits);
        CHECK(all_null(skx::device_view(CallRows{}, have)));
    }
    // ---- the whole record: consensus output x change list x call rows x the call's list, each unbound (8) or with any set of columns
    BatchOut have;
    have.cons = dev_w + 15;
    have.chg = make_events(dev_w, dev_l, 0u, 0u, 5u, 7u, false);
    have.call = make_rows(dev_w, dev_l, 7u);
    have.call_ev = make_events(dev_w, dev_l, 5u, 1u, 5u, 7u, true);
    for (int cons = 0; cons < 2; ++cons)
        for (unsigned chg = 0; chg <= 8; ++chg)
            for (unsigned call = 0; call <= 8; ++call)
                for (unsigned cev = 0; cev <= 8; ++cev) {
                    BatchOut want;
                    if (cons) want.cons = host_w + 15;
                    if (chg < 8) want.chg = make_events(host_w, host_l, 0u, 0u, 9u, chg, false);
                    if (call < 8) want.call = make_rows(host_w, host_l, call);
                    if (cev < 8) want.call_ev = make_events(host_w, host_l, 5u, 1u, 3u, cev, true);
                    const bool codes = (chg < 8 && (chg & 4u)) || (call < 8 && (call & 4u)) || (cev < 8 && (cev & 4u));
                    CHECK(want.wants_vote() == (cons || codes));
                    CHECK(want.wants_call() == (call < 8 || cev < 8));
                    CHECK(want.any() == (cons || chg < 8 || call < 8 || cev < 8));
                    const BatchOut v = skx::device_view(want, have);
                    CHECK(v.cons == ((cons || codes) ? have.cons : nullptr));  // (the votes of a list of codes need a place too)
                    if (chg < 8) check_events_view(want.chg, have.chg, v.chg, chg, false);
                    else CHECK(all_null(v.chg));
                    if (call < 8) check_rows_view(have.call, v.call, call);
                    else CHECK(all_null(v.call));
                    if (cev < 8) check_events_view(want.call_ev, have.call_ev, v.call_ev, cev, true);
                    else CHECK(all_null(v.call_ev));
                    CHECK(v.any() == want.any() && v.wants_call() == want.wants_call() && v.wants_vote() == want.wants_vote());
                    BatchOut b = v;
                    b.set_batch(77u);
                    CHECK(b.chg.n_batch == 77u && b.call_ev.n_batch == 77u && b.chg.cap == v.chg.cap && b.call_ev.cap == v.call_ev.cap);
                }
    {
        const BatchOut v = skx::device_view(BatchOut{}, have);
        CHECK(!v.any() && !v.wants_vote() && !v.wants_call() && !v.cons && all_null(v.chg) && all_null(v.call) && all_null(v.call_ev));
        const BatchOut none = skx::device_view(BatchOut{}, BatchOut{});
        CHECK(!none.any() && all_null(none.chg) && all_null(none.call) && all_null(none.call_ev));
    }
    // ---- widths: passed in by whoever allocates, copies or gathers
    const skx::RowWidths cw = skx::change_widths(3u, 5u, 4u), kw = skx::call_widths(5u, 4u), plain = skx::change_widths(1u, 5u, 0u);
    CHECK(cw.idx == 15u && cw.codes == 12u);
    CHECK(kw.idx == 5u && kw.codes == 4u);
    CHECK(plain.idx == 5u && plain.codes == 0u);  // (no genotype table: no codes column)
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}

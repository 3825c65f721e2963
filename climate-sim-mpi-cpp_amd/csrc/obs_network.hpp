// obs_network.hpp — the observation network as the three host units behind it see it: ensemble_obs.cpp (the network
// itself: create, values, mask, observe, fetch, the logs), ensemble_analysis.cpp (the analyses that run on one) and
// ensemble_obs_impact.cpp (the forecast impact).  Internal: csim_obs_network is opaque in csim.h, so nothing here is
// part of the ABI.  Host only, behind ensemble_host.hpp.
#pragma once
#include <algorithm>
#include <vector>

#include "ensemble_host.hpp"

namespace csim {

// a lookup on the device (LocalTiles, LetkfLookup): its starts, then its plan positions
struct DeviceLookup {
    DeviceBuf buf;
    Staging stage;
    size_t pos_at = 0;  // where the plan positions start, bytes
    int key = 0;        // what it was built for (a tile, a spacing; 0: none)
    void release() { buf.release(), stage.release(); }
    const int* cstart() const { return buf_at<int>(buf.p, 0); }
    const int* cpos() const { return buf_at<int>(buf.p, pos_at); }
    int upload(const std::vector<int>& start, const std::vector<int>& pos, int k, hipStream_t st) {
        const size_t at = up(sizeof(int) * start.size()), bytes = up(at + sizeof(int) * pos.size());
        void* staged = nullptr;
        CSIM_TRY(stage.acquire(bytes, &staged));
        std::copy(start.begin(), start.end(), buf_at<int>(staged, 0));
        std::copy(pos.begin(), pos.end(), buf_at<int>(staged, at));
        key = 0;  // from here on the last lookup is being replaced (after its readers)
        CSIM_TRY(buf.reserve(bytes, st));
        CSIM_TRY(stage.send(buf.p, bytes, st));
        key = k, pos_at = at;
        return CSIM_OK;
    }
};

}  // namespace csim

struct csim_obs_network : csim::AssimPlan {   // the plan: nobs, nlevels, lx, ly, off, idx, pi, pj
    csim_ensemble* e = nullptr;
    int log_cycles = 0, ntaps = 0, tmax = 0;  // ntaps, tmax: a linear network's taps in all, the most of one observation
    std::vector<csim::AssimBatch> batches;    // its launches for batches_m forecast members (made at the first analysis)
    int batches_m = 0;
    csim::ObsLayout l{};
    csim::DeviceBuf dev;
    csim::Staging stage;                // of set_values
    csim::Staging mstage;               // of set_active
    bool has_values = false, has_truth = false, has_diag = false;
    bool masked = false;                // the mask on the device has an inactive observation (else it is not read)
    bool analysed = false, screened = false;  // there was an analysis; the last one launched the screening
    int cycles = 0;                     // records in both logs
    bool last_recorded = false;         // the last analysis was a recorded one: bg and the status bytes are its own
    // the capture of csim_obs_network_impact_capture, made at the first capture and kept until destroy
    struct Impact {
        csim::DeviceBuf pert;           // M doubles per plan position: a_k
        csim::DeviceBuf aux;            // dn (plan order), J (input order), the status snapshot (plan order)
        csim::DeviceBuf w;              // the weight of the last csim_ensemble_obs_impact, dense
        csim::Staging wstage;
        bool valid = false;
        int M = 0, t = 0;               // its forecast members: M of them, member t left out (t = B: none)
        void release() { pert.release(), aux.release(), w.release(), wstage.release(); }
    } imp;
    // the local analysis (csim_ensemble_assimilate_local), made at the first one and kept until destroy
    struct Local {
        int max_local = -1;             // the most window rectangles over one cell (-1: not counted yet)
        csim::DeviceBuf prior;          // M doubles per plan position: h_{o,k}
        csim::DeviceLookup tiles;       // the lookup (LocalTiles), its key the tile
        int ntx = 0, nty = 0;           // of the lookup on the device
        void release() { prior.release(), tiles.release(); }
    } loc;
    // the LETKF (csim_ensemble_assimilate_letkf): the lookup of the last spacing, made when the spacing is another one
    // and kept until destroy; the observation priors are those of the local analysis (loc.prior)
    struct Letkf {
        csim::DeviceLookup nodes;       // the lookup (LetkfLookup), its key the spacing
        void release() { nodes.release(); }
    } letkf;
    // time slots and held rows (csim_obs_network_set_slots, _hold, csim_ensemble_assimilate_etkf_held): nothing here is
    // allocated before the first set_slots (the list) or the first hold (the rows)
    struct Held {
        std::vector<int> start;         // per slot, one more than slots: where its plan positions start in the list;
                                        // empty: every observation in slot 0, and there is no list
        csim::DeviceLookup list;        // starts and plan positions, grouped by slot, increasing within one; key 1: made
        unsigned long long present = 1; // bit s: slot s occurs (csim_obs_slots_present)
        unsigned long long held = 0;    // bit s: slot s has been held since set_slots, the last held analysis, or a
                                        // hold with another (M, t)
        unsigned long long seen = 0;    // bit s: slot s has been observed since set_slots or set_values
        csim::DeviceBuf rows;           // M doubles per plan position: h_{o,k} at its slot's time
        int M = 0, t = 0;               // of the rows (M = 0: there are none)
        bool last = false;              // the network's last analysis was a held one
        bool done = false;              // the rows are those a held analysis left, and there was no hold since
        bool all_held() const { return (held & present) == present; }
        void release() { list.release(), rows.release(); }
    } hold;
    size_t imp_dn() const { return 0; }
    size_t imp_out() const { return csim::up(sizeof(double) * nobs); }
    size_t imp_snap() const { return 2 * csim::up(sizeof(double) * nobs); }
    size_t imp_bytes() const { return imp_snap() + csim::up(nobs); }
    template <class T> T* at(size_t byte) const { return csim::buf_at<T>(dev.p, byte); }
    csim::ObsArgs args() const {
        csim::ObsArgs a{};
        a.nobs = nobs;
        a.i = at<int>(l.i), a.j = at<int>(l.j), a.idx = at<int>(l.idx), a.pos = at<int>(l.pos);
        a.r = at<double>(l.r), a.sr = at<double>(l.sr);
        a.y = at<double>(l.y), a.xt = at<double>(l.xt);
        a.bg = at<double>(l.bg), a.post = at<double>(l.post), a.part = at<double>(l.part);
        if (ntaps) a.tstart = at<int>(l.tstart), a.toff = at<int>(l.toff), a.tw = at<double>(l.tw);
        return a;
    }
    ~csim_obs_network() { dev.release(), stage.release(), mstage.release(), imp.release(), loc.release(), letkf.release(), hold.release(); }
};

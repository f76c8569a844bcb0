// handover.h -- what a k-block keeps between two dftk_mi_lobpcg calls.  Host only.
//
// The general driver leaves its A X (in the k-block's LOBPCG workspace) and remembers where it put the returned X.  A
// Gamma-real density pass over that very X writes its y-planes (stage-B output) into `planes` instead of the recycled
// scratch.  The next call, if the caller promises that it starts from the returned X, takes both:
// A_new X = A_old X + (V_new - V_old) X, the difference applied from the planes where they are usable.
//
//   event                                     kept A X   promise     returned X   planes
//   keep + returned (exit, general driver)    set        -           set          -
//   promise(on)                               -          on && kept  -            -
//   take (a call binds the workspace)         dropped    dropped     dropped      off
//   density pass over the returned X          -          -           -            on (groups marked as they run)
//   density pass that keeps nothing           -          -           -            off
//   consume (start from the planes)           -          -           -            off
//   forget_planes (new shard / format)        -          -           dropped      off
//   forget (new projectors)                   dropped    dropped     dropped      off
//   decline (no room for the buffer)          -          -           -            never on again
//
// take hands the kept A X out only if it was promised, the shape is equal and the workspace stays where it is; the planes
// only with the A X, and only if they are eligible, on, and were written for M bands under today's launch-group size.
#pragma once
#include <algorithm>
#include <vector>
#include "devbuf.h"

typedef double2 cd;

struct LobHandover {
    // The buffers are public: when they are allocated and filled is their users' business (lobpcg.cpp, gamma_kernels.hip);
    // they are freed with the k-block.  Everything else changes through the member functions only.
    DevTable<double> V_kept;      // [nz*ny*nxp] snapshot of the bound potential at the exit that kept A X
    DevTable<double> dV;          // [nz*ny*nxp] scratch: V_new - V_old
    DevTable<cd> planes;          // pair p in slot p, nzx * ny * nxp elements each (allocated on first use)

    struct Taken {
        cd* AX = nullptr;         // the kept A X (borrowed: points into the LOBPCG workspace), or null
        int64_t ld = 0;
        bool planes = false;      // the y-planes of the returned X are usable (never without AX)
    };

    // dftk_mi_kblock_reuse_AX: X0 of the next call IS the X the last one returned.  One-shot; true only while an A X is kept.
    void promise(bool on) { promised_ = on && kept_ != nullptr; }

    // Once per call, by whichever driver binds the workspace (every call overwrites it): nothing is kept afterwards.
    Taken take(int M, int64_t N, bool workspace_moves, bool planes_eligible, int fft_batch) {
        Taken t;
        if (promised_ && kept_M_ == M && kept_N_ == N && !workspace_moves) {
            t.AX = kept_;
            t.ld = kept_ld_;
            t.planes = planes_eligible && on_ && planes != nullptr && back_M_ == M && batch_ == fft_batch &&
                       valid_.size() == (size_t)(M + 1) / 2;
        }
        promised_ = false;
        kept_ = nullptr;
        forget_planes();
        return t;
    }

    // exit of the general driver: A X sorted like the returned X (the caller has snapshot the potential into V_kept) ...
    void keep(cd* AX, int64_t ld, int M, int64_t N) {
        kept_ = AX;
        kept_ld_ = ld;
        kept_M_ = M;
        kept_N_ = N;
    }
    // ... and where the returned X lives (un-sharded Gamma-real blocks only)
    void returned(const cd* X, int64_t ld, int M) {
        back_X_ = X;
        back_ld_ = ld;
        back_M_ = M;
    }

    void forget() {               // new projectors: the kept A X belongs to the old nonlocal term
        kept_ = nullptr;
        promised_ = false;
        forget_planes();
    }
    void forget_planes() {        // new shard or format: the planes belong to the one the block was returned in
        on_ = false;
        back_X_ = nullptr;
    }

    // ---- density side ----
    // does a pass over nb bands at psi run over the very block the last call returned (and may it keep planes at all)?
    bool pass_keeps_planes(const cd* psi, int64_t ld, int nb) const {
        return !declined_ && back_X_ != nullptr && back_X_ == psi && back_ld_ == ld && back_M_ == nb;
    }
    // such a pass starts: no pair written yet; fft_batch sets the launch groups the valid flags follow
    void planes_begin(int nb, int fft_batch) {
        valid_.assign((size_t)(nb + 1) / 2, 0);
        batch_ = fft_batch;
        on_ = true;
    }
    void planes_mark(int p0, int n) { std::fill_n(valid_.begin() + p0, n, (char)1); }   // a launch group ran
    // a pass that keeps nothing ran: what is in the slots belongs to another block or shape (the returned X is remembered:
    // a later pass over it may keep planes again)
    void planes_off() { on_ = false; }
    // the start from the planes: which pairs were written (the rest the caller fills itself); the planes are spent
    const std::vector<char>& planes_consume() {
        on_ = false;
        return valid_;
    }
    void planes_decline() { declined_ = true; }   // the device had no room for the buffer: off for this block, for good

    // A X of the current pair for dftk_mi_lobpcg_last_AX (borrowed; null for half-format blocks, which are not handed out)
    void set_last_AX(cd* AX) { last_AX_ = AX; }
    cd* last_AX() const { return last_AX_; }

private:
    cd* last_AX_ = nullptr;
    cd* kept_ = nullptr;          // the kept A X: borrowed (into the LOBPCG workspace)
    int kept_M_ = 0;
    int64_t kept_N_ = 0, kept_ld_ = 0;
    bool promised_ = false;
    const cd* back_X_ = nullptr;  // the returned X: borrowed; null: no general-driver call since, or not eligible
    int64_t back_ld_ = 0;
    int back_M_ = 0;
    bool on_ = false;             // the slots of `planes` belong to back_X_: valid_[p] tells which were written
    bool declined_ = false;       // no planes for this block, ever
    int batch_ = 0;               // fft_batch of the density pass (the launch groups valid_ follows)
    std::vector<char> valid_;     // [(back_M_ + 1) / 2]
};

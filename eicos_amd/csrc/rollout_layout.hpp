// A rollout's three device buffers and the trajectory a handle keeps of it (api.cpp: rollout_run and the calls that read a rollout
// back), described once: from what the call knows before its first allocation come the byte offset of every part and the total of
// every buffer, so that a reserve and the pointers under it cannot disagree.  Host only, and no HIP symbol, as resources.hpp and
// call_arrays.hpp: tests/host/rollout_layout_check.cpp compiles this header on its own.
//   d_roll  = [RolloutDev | theta [B][T + 1][k] | u [B][T][r] | w [B][T][k], where the caller gives one | two theta rows of the batch
//              [2][B][k], which take turns on the path that is not fused | codes [B][T] | iters [B][T]], the last two of ints
//   d_rollJ = [AdjointDev of the fused launch | J [B][T][r][k] | res [B][T][r] | one step's J [B][r][k] and res [B][r], which the path
//              that is not fused moves into the two trajectories]: made by a rollout that records its Jacobians (sens), and kept
//   d_rollW = the rows of a recording rollout (launch.hpp: AdjointDev::x_rec): the whole record, B T rows as lay_records lays them
//              out, and -- the ONE statement of that rule -- one step's B rows behind it where the rollout is not fused
// Every part of the first two starts on a 64-byte boundary; a part without width takes no bytes and has no address.  The record is
// doubles only and packed, so that its total is the product its refusal names; its parts of no width keep an address (the launchers
// refuse a NULL array).
#pragma once

#include <climits>
#include <cstddef>
#include <string>

namespace eicos {

constexpr size_t ROLLOUT_HEADER = 128; // bytes kept for the launch record in front of d_roll and d_rollJ (api.cpp: MAP_HEADER)

// Recorded rows -- one step's, or the whole record --: six arrays one behind the other, [rows][width[q]] each
struct RecordRows {
    double *Wc, *Wh, *Wb, *x, *y, *z; size_t width[6];
    double *part(int q) const { double *const a[6] = {Wc, Wh, Wb, x, y, z}; return a[q]; }
};
// The one layout of recorded rows: `rows` rows from byte `at` of their buffer, widths per row [Wc r n | Wh r m | Wb r p | x n | y p | z m]
struct RecordLayout {
    size_t rows = 0, width[6] = {}, at[6] = {}, end = 0; // (rows = 0: no such rows, and no bytes)
    RecordRows in(void *base) const {
        double *a[6];
        for (int q = 0; q < 6; q++) a[q] = static_cast<double *>(static_cast<void *>(static_cast<char *>(base) + at[q]));
        return RecordRows{a[0], a[1], a[2], a[3], a[4], a[5], {width[0], width[1], width[2], width[3], width[4], width[5]}};
    }
    // row t of instance b of a record of `steps` steps, in bytes from the buffer's start: rows are [batch][steps]
    size_t row_at(int q, size_t b, size_t t, size_t steps) const { return at[q] + (b * steps + t) * width[q] * sizeof(double); }
};
inline RecordLayout lay_records(size_t at, size_t rows, size_t r, size_t n, size_t m, size_t p) {
    RecordLayout L;
    const size_t width[6] = {r * n, r * m, r * p, n, p, m};
    L.rows = rows;
    for (int q = 0; q < 6; q++) { L.width[q] = width[q]; L.at[q] = at; at += rows * width[q] * sizeof(double); }
    L.end = at;
    return L;
}

// What rollout_run knows before its first allocation.  recording implies sens.
struct RolloutShape {
    size_t B, T, k, r, n, m, p; // batch, steps, the parameter and output counts, the pattern's sizes
    bool w, sens, recording, fused;
};
// "batch * steps must fit an int" (the kernels index a trajectory's rows with one); empty: the shape is fine
inline std::string rollout_shape_fault(const RolloutShape &s) {
    if (s.sens && s.B * s.T > (size_t)INT_MAX) return "rollout_jacobian: batch * steps must fit an int";
    return std::string();
}

// the device pointers of one rollout call (NULL: the call has no such part)
struct RolloutArrays {
    void *roll_rec, *adj_rec;                           // the records of the launch in front of d_roll and d_rollJ
    double *theta, *u, *w, *cur; int *codes, *iters;    // d_roll
    double *J, *res, *J1, *res1;                        // d_rollJ (sens)
    RecordRows W, W1;                                   // d_rollW (recording): the whole record; one step's rows (not fused)
};
struct RolloutLayout {
    struct Part { // where a part starts in its buffer and what it takes
        size_t at = 0, bytes = 0;
        template <class T> T *in(void *base) const { return bytes ? static_cast<T *>(static_cast<void *>(static_cast<char *>(base) + at)) : nullptr; }
    };
    Part roll_rec, theta, u, w, cur, codes, iters; size_t roll_bytes = 0;  // d_roll
    Part adj_rec, J, res, J1, res1; size_t rollJ_bytes = 0;                 // d_rollJ (sens)
    RecordLayout record, step; size_t rollW_bytes = 0;                      // d_rollW (recording); step.rows != 0 exactly where not fused

    explicit RolloutLayout(const RolloutShape &s) {
        const size_t D = sizeof(double), I = sizeof(int), BT = s.B * s.T;
        size_t end = 0;
        const auto put = [&end](Part &q, size_t bytes) { // the part behind the ones put so far, on its boundary
            if (!bytes) return;
            q.at = (end + 63) & ~(size_t)63; q.bytes = bytes; end = q.at + bytes;
        };
        put(roll_rec, ROLLOUT_HEADER); put(theta, s.B * (s.T + 1) * s.k * D); put(u, BT * s.r * D); put(w, s.w ? BT * s.k * D : 0);
        put(cur, 2 * s.B * s.k * D); put(codes, BT * I); put(iters, BT * I);
        roll_bytes = end;
        if (!s.sens) return;
        end = 0;
        put(adj_rec, ROLLOUT_HEADER); put(J, BT * s.r * s.k * D); put(res, BT * s.r * D); put(J1, s.B * s.r * s.k * D); put(res1, s.B * s.r * D);
        rollJ_bytes = end;
        if (!s.recording) return;
        record = lay_records(0, BT, s.r, s.n, s.m, s.p);
        step = lay_records(record.end, s.fused ? 0 : s.B, s.r, s.n, s.m, s.p);
        rollW_bytes = step.end;
    }
    // every pointer of the call, given the three buffers (each of at least its total; one that has no bytes is not looked at)
    RolloutArrays in(void *roll, void *rollJ, void *rollW) const {
        RolloutArrays a{};
        a.roll_rec = roll_rec.in<void>(roll); a.theta = theta.in<double>(roll); a.u = u.in<double>(roll); a.w = w.in<double>(roll);
        a.cur = cur.in<double>(roll); a.codes = codes.in<int>(roll); a.iters = iters.in<int>(roll);
        a.adj_rec = adj_rec.in<void>(rollJ); a.J = J.in<double>(rollJ); a.res = res.in<double>(rollJ); a.J1 = J1.in<double>(rollJ); a.res1 = res1.in<double>(rollJ);
        if (record.rows) a.W = record.in(rollW);
        if (step.rows) a.W1 = step.in(rollW);
        return a;
    }
};

// The trajectory a handle holds between eicos_batch_rollout_jacobian and the calls that read it back: what was recorded, under which
// (k, r), plant descriptor (Plant: launch.hpp, PlantMapDev) and map generation, and whether with its rows.  The pointers are those of
// the rollout's layout; they are read through the accessors, which every reader calls behind fault().
template <class Plant> struct HeldTrajectory {
    int steps = 0, k = 0, r = 0;  // steps = 0: no trajectory on the handle
    size_t rows = 0;              // batch * steps: the rows of J, res and every part of the record
    Plant plant{};
    unsigned long gen = 0;        // the handle's map generation at that rollout
    bool with_rows = false;       // recorded with its rows (a recording rollout), and the record is still there

    // until this rollout has been enqueued whole: a failure in between leaves no trajectory
    void invalidate() { steps = 0; with_rows = false; }
    // rec = NULL: recording was off
    void hold(size_t batch, int steps_, int k_, int r_, const Plant &plant_, unsigned long map_gen, double *J, double *res, const RecordRows *rec) {
        steps = steps_; k = k_; r = r_; rows = batch * (size_t)steps_; plant = plant_; gen = map_gen;
        J_ = J; res_ = res; with_rows = rec != nullptr;
        if (rec) rec_ = *rec;
    }
    void drop_rows() { with_rows = false; } // the record's buffer goes away (recording switched off); J and res stay
    const double *J() const { return J_; }
    const double *res() const { return res_; }
    const RecordRows &records() const { return rec_; }

    // The trajectory a backward sweep or a read of the record needs, as a message `who` reports; empty: it is there.  map_gen = the
    // handle's count of installs of the parameter, matrix, output, plant and fallback maps; current: the trajectory must belong to
    // the maps now installed.
    std::string fault(const char *who, unsigned long map_gen, bool need_records, bool current = true) const {
        const std::string w(who);
        if (steps == 0) return w + ": the handle holds no Jacobian trajectory (eicos_batch_rollout_jacobian records one)";
        if (current && gen != map_gen) return w + ": a parameter, matrix, output, plant or fallback map was installed after the rollout whose Jacobians the handle holds (setting or clearing per-instance plant values counts as one): run eicos_batch_rollout_jacobian again";
        if (need_records && !with_rows) return w + ": the handle holds no recorded rows: recording was off for the rollout it holds (eicos_batch_set_rollout_recording, then eicos_batch_rollout_jacobian)";
        return std::string();
    }

private:
    double *J_ = nullptr, *res_ = nullptr;
    RecordRows rec_{};
};

} // namespace eicos

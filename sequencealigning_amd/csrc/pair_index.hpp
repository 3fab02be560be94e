// Pair resolution of a batch and the error text of a failed call: the part of
// the host support layer (host_common.hpp) that needs no HIP, for the modules
// that are tested on the CPU (nw_plan_layout.cpp).
#pragma once
#include <cstdint>
#include <string>

namespace saln {

void set_error(const std::string &msg);

// Pair k of a batch: the caller's index lists, or without them the q-major
// grid over n_q x n_db (db-outer, query-inner, as the reference's loop).
struct PairIndex {
    const uint32_t *pair_q, *pair_db;
    uint64_t n_q, n_db;
    // plans: both lists or neither, and without them n_pairs is the whole grid
    bool complete(uint64_t n_pairs) const {
        if (!pair_q != !pair_db) return false;
        if (pair_q || n_pairs == n_q * n_db) return true;
        set_error("all-vs-all needs n_pairs == n_q * n_db");
        return false;
    }
    // false ("pair index out of range") for an index outside the sets
    bool at(uint64_t k, uint64_t *qi, uint64_t *di) const {
        *qi = pair_q ? pair_q[k] : n_q ? k % n_q : 0;
        *di = pair_db ? pair_db[k] : n_q ? k / n_q : 0;
        if (*qi < n_q && *di < n_db) return true;
        set_error("pair index out of range");
        return false;
    }
};

// The lengths of query qi and db record di from the offset tables; false
// ("sequence too long") when one exceeds the engine's limit.
inline bool pair_lengths(const uint64_t *q_off, const uint64_t *db_off, uint64_t qi, uint64_t di,
                         uint64_t limit, uint64_t *lq, uint64_t *ld) {
    *lq = q_off[qi + 1] - q_off[qi];
    *ld = db_off[di + 1] - db_off[di];
    if (*lq <= limit && *ld <= limit) return true;
    set_error("sequence too long");
    return false;
}

}  // namespace saln

// Host build of the termination rule of the five-point RANSAC (e5_confident and the checkpoint sequence of
// mvslam_amd/csrc/five_point.hpp).  Built by tests/test_essential5_confidence.py
//   - as a shared object the tests load with ctypes (the extern "C" functions), compared there with a numpy statement of the rule;
//   - as a stand-alone program (main below), plain and under -fsanitize=address,undefined: the whole grid of the test once more,
//     checked for what the rule must satisfy whatever its rounding -- never with c = 0, monotone in c, in j and in p, always
//     with c = M -- and the checkpoint sequences for their ends, their doubling and their length.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#define MVS_DEV static inline
#include "../../mvslam_amd/csrc/five_point.hpp"

extern "C" {

int e5_confident_host(int c, int M, int j, double p) { return mvs::e5_confident(c, M, j, p) ? 1 : 0; }

// out[c] for c = 0 .. M
void e5_confident_row(int M, int j, double p, uint8_t *out)
{
    for (int c = 0; c <= M; ++c)
        out[c] = mvs::e5_confident(c, M, j, p) ? 1 : 0;
}

// the checkpoints of H hypotheses into out[cap]; returns their number (also when it exceeds cap)
int e5_checkpoints(int H, int *out, int cap)
{
    int n = 0;
    for (int T = mvs::e5_checkpoint_first(H);; T = mvs::e5_checkpoint_next(T, H)) {
        if (n < cap)
            out[n] = T;
        ++n;
        if (T >= H)
            break;
    }
    return n;
}

}  // extern "C"

int main()
{
    const int Ms[] = {8, 9, 150, 4096};
    const double ps[] = {0.5, 0.95, 0.99, 0.999999};
    long bad = 0, cases = 0, stops = 0;
    for (int M : Ms) {
        std::vector<uint8_t> row(M + 1), prev_j(M + 1), prev_p(M + 1);
        for (int pi = 3; pi >= 0; --pi)      // p descending: a pair that stops at a higher confidence stops at a lower one
            for (int j = 0; j <= 10; ++j) {
                e5_confident_row(M, j, ps[pi], row.data());
                bad += row[0] != 0;
                bad += row[M] != 1;          // q = 0 exactly
                for (int c = 1; c <= M; ++c)
                    bad += row[c] < row[c - 1];
                if (j > 0)
                    for (int c = 0; c <= M; ++c)
                        bad += row[c] < prev_j[c];
                prev_j = row;
                cases += M + 1;
                for (int c = 0; c <= M; ++c)
                    stops += row[c];
            }
        for (int j = 0; j <= 10; ++j) {
            e5_confident_row(M, j, ps[3], prev_p.data());
            for (int pi = 2; pi >= 0; --pi) {
                e5_confident_row(M, j, ps[pi], row.data());
                for (int c = 0; c <= M; ++c)
                    bad += row[c] < prev_p[c];
                prev_p = row;
            }
        }
    }
    const int Hs[] = {1, 63, 64, 65, 128, 129, 1000, 10000, 2147483647};
    long seqs = 0;
    for (int H : Hs) {
        int T[40];
        const int n = e5_checkpoints(H, T, 40);
        bad += n < 1 || n > 40;
        if (n < 1 || n > 40)
            continue;
        bad += T[0] != (H < 64 ? H : 64);
        bad += T[n - 1] != H;
        for (int k = 1; k < n; ++k)
            bad += !(T[k] == 2 * (long)T[k - 1] || (k == n - 1 && T[k] < 2 * (long)T[k - 1] && T[k] > T[k - 1]));
        ++seqs;
    }
    printf("e5_confident cases=%ld stops=%ld sequences=%ld bad=%ld\n", cases, stops, seqs, bad);
    return bad == 0 ? 0 : 1;
}

// Stand-alone check of the host side of the particle entry points (tlab_amd/csrc/particles_host.hpp): the argument checks and the layout of the
// sort's scratch array, with no device and no HIP header, meant to be built with the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/particles_host_check.cpp -o particles_host_check && ./particles_host_check
// Exit status 0 and "particles_host_check ok" when every case gives the code it must.
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "../tlab_amd/csrc/particles_host.hpp"

using namespace tlab;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    std::string why;
    int bcs = -7;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- tlab_dns_set_particles ----
    for (int t : {4, 5, 6}) EXPECT(particle_check_settings(t, -1, 1.0, 0.0, &bcs, why) == TLAB_EUNSUPPORTED && bcs == -7 && !why.empty());
    for (int t : {-1, 3, 7, 1 << 30}) EXPECT(particle_check_settings(t, -1, 1.0, 0.0, &bcs, why) == TLAB_EINVAL && bcs == -7);
    EXPECT(particle_check_settings(TLAB_PART_TRACER, 3, 0.0, 0.0, &bcs, why) == TLAB_EINVAL && bcs == -7);
    EXPECT(particle_check_settings(TLAB_PART_INERTIA, -1, 0.0, 0.0, &bcs, why) == TLAB_EINVAL && bcs == -7);
    EXPECT(particle_check_settings(TLAB_PART_INERTIA, -1, -1.0, 0.0, &bcs, why) == TLAB_EINVAL);
    EXPECT(particle_check_settings(TLAB_PART_INERTIA, -1, nan, 0.0, &bcs, why) == TLAB_EINVAL);
    EXPECT(particle_check_settings(TLAB_PART_INERTIA, -1, 1.0, inf, &bcs, why) == TLAB_EINVAL);
    EXPECT(particle_check_settings(TLAB_PART_TRACER, -1, 0.0, nan, &bcs, why) == TLAB_EINVAL && bcs == -7);
    EXPECT(particle_check_settings(TLAB_PART_TRACER, -1, 0.0, 0.0, &bcs, why) == TLAB_OK && bcs == TLAB_PART_BCS_NONE);
    EXPECT(particle_check_settings(TLAB_PART_INERTIA, -1, 0.5, 0.1, &bcs, why) == TLAB_OK && bcs == TLAB_PART_BCS_SPECULAR);
    EXPECT(particle_check_settings(TLAB_PART_INERTIA, TLAB_PART_BCS_STICK, 0.5, 0.1, &bcs, why) == TLAB_OK && bcs == TLAB_PART_BCS_STICK);
    EXPECT(particle_check_settings(TLAB_PART_NONE, 99, nan, nan, &bcs, why) == TLAB_OK && bcs == TLAB_PART_BCS_NONE);      // type 0 reads nothing else
    EXPECT(particle_columns(TLAB_PART_TRACER) == 3 && particle_columns(TLAB_PART_INERTIA) == 6);

    // ---- tlab_dns_substep_particle ----
    double a = 0.0;
    int node = 1;
    std::vector<double *> q(3, &a), l6(6, &a), l3(3, &a), hole(6, &a);
    hole[4] = nullptr;
    EXPECT(particle_check_substep(false, 0, 1e-3, 1.0, 1, q.data(), l3.data(), l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, -1, q.data(), l3.data(), l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, PARTICLE_NP_MAX + 1, q.data(), l3.data(), l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, std::numeric_limits<long long>::max(), q.data(), l3.data(), l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, nan, 1.0, 1, q.data(), l3.data(), l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, 0, nullptr, nullptr, nullptr, nullptr, why) == TLAB_OK);      // np = 0 reads no pointer
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, 1, nullptr, l3.data(), l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, 1, q.data(), nullptr, l3.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, 1, q.data(), l3.data(), nullptr, &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, 1, q.data(), l3.data(), l3.data(), nullptr, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 6, 1e-3, 1.0, 1, q.data(), hole.data(), l6.data(), &node, why) == TLAB_EINVAL);
    EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, 1, q.data(), hole.data(), l3.data(), &node, why) == TLAB_OK);      // a tracer reads three columns: l3-sized arrays are enough
    {   // exactly three entries on the heap: a read of a fourth would be caught
        std::unique_ptr<double *[]> t3(new double *[3]{&a, &a, &a});
        EXPECT(particle_check_substep(true, 3, 1e-3, 1.0, PARTICLE_NP_MAX, t3.get(), t3.get(), t3.get(), &node, why) == TLAB_OK);
    }

    // ---- the scratch of tlab_dns_particle_sort ----
    ParticleSortLayout L;
    EXPECT(particle_sort_layout(-1, 0, &L, why) == TLAB_EINVAL);
    EXPECT(particle_sort_layout(PARTICLE_NP_MAX + 1, 0, &L, why) == TLAB_EINVAL);
    EXPECT(particle_sort_layout(10, ~(size_t)0, &L, why) == TLAB_EINVAL);
    for (long long np : {0LL, 1LL, 63LL, 64LL, 65LL, 1000LL, 1LL << 24, 67108864LL, PARTICLE_NP_MAX}) {
        for (size_t sb : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)123457, (size_t)1 << 40}) {
            EXPECT(particle_sort_layout(np, sb, &L, why) == TLAB_OK);
            const size_t n = (size_t)np, parts[6] = {L.keys_in, L.keys_out, L.idx_in, L.idx_out, L.column, L.sort};
            const size_t sizes[6] = {4 * n, 4 * n, 4 * n, 4 * n, 8 * n, sb ? sb : 1};
            for (int i = 0; i < 6; ++i) {
                EXPECT(parts[i] % PARTICLE_SCRATCH_ALIGN == 0);
                EXPECT(parts[i] + sizes[i] <= (i < 5 ? parts[i + 1] : L.total));      // no part reaches into the next, the last not beyond the total
            }
            EXPECT(L.total % PARTICLE_SCRATCH_ALIGN == 0 && L.total <= 24 * n + sb + 7 * PARTICLE_SCRATCH_ALIGN);
        }
    }
    // a real scratch array of the size the layout asks for: every part written end to end (the sanitizer watches the bounds)
    {
        const long long np = 1000;
        EXPECT(particle_sort_layout(np, 4099, &L, why) == TLAB_OK);
        std::vector<unsigned char> mem(L.total + PARTICLE_SCRATCH_ALIGN);
        unsigned char *base = mem.data() + (PARTICLE_SCRATCH_ALIGN - reinterpret_cast<size_t>(mem.data()) % PARTICLE_SCRATCH_ALIGN) % PARTICLE_SCRATCH_ALIGN;
        for (size_t off : {L.keys_in, L.keys_out, L.idx_in, L.idx_out})
            for (long long p = 0; p < np; ++p) reinterpret_cast<unsigned *>(base + off)[p] = (unsigned)p;
        for (long long p = 0; p < np; ++p) reinterpret_cast<double *>(base + L.column)[p] = (double)p;
        for (size_t b = 0; b < 4099; ++b) (base + L.sort)[b] = 1;
        long long tag = 1;
        EXPECT(particle_check_sort(true, 3, np, l3.data(), l3.data(), &node, &tag, base, (long long)L.total, L.total, why) == TLAB_OK);
        EXPECT(particle_check_sort(true, 3, np, l3.data(), l3.data(), &node, &tag, base, (long long)L.total - 1, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(true, 3, np, l3.data(), l3.data(), &node, &tag, base, -5, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(true, 3, np, l3.data(), l3.data(), &node, &tag, base + 8, (long long)L.total, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(false, 0, np, l3.data(), l3.data(), &node, &tag, base, (long long)L.total, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(true, 3, np, l3.data(), l3.data(), nullptr, &tag, base, (long long)L.total, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(true, 3, np, l3.data(), l3.data(), &node, nullptr, base, (long long)L.total, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(true, 6, np, hole.data(), l6.data(), &node, &tag, base, (long long)L.total, L.total, why) == TLAB_EINVAL);
        EXPECT(particle_check_sort(true, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, why) == TLAB_OK);
    }
    // ---- the bits of the key ----
    EXPECT(particle_key_bits(1) == 1 && particle_key_bits(2) == 1 && particle_key_bits(3) == 2 && particle_key_bits(1920) == 11);
    EXPECT(particle_key_bits(1ULL << 27) == 27 && particle_key_bits((1ULL << 27) + 1) == 28 && particle_key_bits(0x7fffffffULL) == 31);
    EXPECT(particle_key_bits(~0ULL) == 32);
    for (unsigned long long n : {1ULL, 2ULL, 1000ULL, 20ULL * 12 * 8, 70ULL * 33 * 9, 1ULL << 27, 0x7fffffffULL})
        EXPECT(n - 1 < (1ULL << particle_key_bits(n)));      // the largest cell number fits

    // ---- tlab_dns_field_to_particle ----
    {
        const double f = 0.0;
        std::vector<const double *> fl(9, &f), fhole(9, &f);
        std::vector<double *> out(9, &a), ohole(9, &a);
        fhole[8] = nullptr; ohole[0] = nullptr;
        EXPECT(particle_check_sample(false, 1, fl.data(), 1, l3.data(), &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 0, fl.data(), 1, l3.data(), &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, -3, fl.data(), 0, l3.data(), &node, out.data(), why) == TLAB_EINVAL);      // nvar is read before np = 0 returns
        EXPECT(particle_check_sample(true, 1, fl.data(), -1, l3.data(), &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 1, fl.data(), PARTICLE_NP_MAX + 1, l3.data(), &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 9, nullptr, 0, nullptr, nullptr, nullptr, why) == TLAB_OK);                 // np = 0 reads no pointer
        EXPECT(particle_check_sample(true, 9, nullptr, 1, l3.data(), &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 9, fl.data(), 1, nullptr, &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 9, fl.data(), 1, l3.data(), nullptr, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 9, fl.data(), 1, l3.data(), &node, nullptr, why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 9, fhole.data(), 1, l3.data(), &node, out.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 9, fl.data(), 1, l3.data(), &node, ohole.data(), why) == TLAB_EINVAL);
        EXPECT(particle_check_sample(true, 8, fhole.data(), 1, l3.data(), &node, out.data(), why) == TLAB_OK);          // the hole is the ninth
        EXPECT(particle_check_sample(true, 9, fl.data(), 1, hole.data(), &node, out.data(), why) == TLAB_OK);           // positions: three columns
        std::unique_ptr<const double *[]> f1(new const double *[1]{&f});      // exactly nvar entries on the heap
        std::unique_ptr<double *[]> o1(new double *[1]{&a});
        EXPECT(particle_check_sample(true, 1, f1.get(), PARTICLE_NP_MAX, l3.data(), &node, o1.get(), why) == TLAB_OK);
    }
    // ---- tlab_dns_particle_to_field ----
    EXPECT(particle_check_deposit(false, 1, l3.data(), &node, &a, why) == TLAB_EINVAL);
    EXPECT(particle_check_deposit(true, -1, l3.data(), &node, &a, why) == TLAB_EINVAL);
    EXPECT(particle_check_deposit(true, PARTICLE_NP_MAX + 1, l3.data(), &node, &a, why) == TLAB_EINVAL);
    EXPECT(particle_check_deposit(true, 0, nullptr, nullptr, nullptr, why) == TLAB_EINVAL);      // the field is zero-filled even then
    EXPECT(particle_check_deposit(true, 0, nullptr, nullptr, &a, why) == TLAB_OK);
    EXPECT(particle_check_deposit(true, 1, nullptr, &node, &a, why) == TLAB_EINVAL);
    EXPECT(particle_check_deposit(true, 1, l3.data(), nullptr, &a, why) == TLAB_EINVAL);
    EXPECT(particle_check_deposit(true, 1, l3.data(), &node, nullptr, why) == TLAB_EINVAL);
    EXPECT(particle_check_deposit(true, PARTICLE_NP_MAX, hole.data(), &node, &a, why) == TLAB_OK);
    // ---- tlab_dns_set_trajectories ----
    {
        std::vector<std::pair<long long, int>> table{{77, 7}};
        const std::vector<std::pair<long long, int>> kept = table;
        const long long good[5] = {40, 3, 1LL << 40, 1, 17}, twice[4] = {5, 9, 5, 2}, zero[3] = {4, 0, 2}, negative[2] = {-1, 3};
        EXPECT(particle_trajectory_table(false, 5, good, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, -1, good, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, PARTICLE_NTRAJ_MAX + 1, good, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, 5, nullptr, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, 4, twice, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, 3, zero, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, 2, negative, &table, why) == TLAB_EINVAL && table == kept);
        EXPECT(particle_trajectory_table(true, 5, good, &table, why) == TLAB_OK && table.size() == 5);
        const std::vector<std::pair<long long, int>> want{{1, 4}, {3, 2}, {17, 5}, {40, 1}, {1LL << 40, 3}};      // sorted by tag, rows 1-based
        EXPECT(table == want);
        EXPECT(particle_trajectory_table(true, 2, twice, &table, why) == TLAB_OK && table.size() == 2);         // (only the first two are read)
        EXPECT(particle_trajectory_table(true, 0, nullptr, &table, why) == TLAB_OK && table.empty());
    }
    // ---- tlab_dns_trajectories_accumulate ----
    {
        const double f = 0.0;
        float tr = 0.0f;
        long long tag = 1;
        std::vector<const double *> fl(2, &f), fhole(2, &f);
        fhole[1] = nullptr;
        auto chk = [&](bool has, int nc, long long ntraj, double rtime, long long counter, long long nsave, long long np, double *const *lq,
                       const int *nodes, const long long *tags, int nvar, const double *const *fields, const float *traj) {
            return particle_check_trajectories(has, nc, ntraj, rtime, counter, nsave, np, lq, nodes, tags, nvar, fields, traj, why);
        };
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_OK);
        EXPECT(chk(true, 6, 4, inf, 7, 7, PARTICLE_NP_MAX, l6.data(), &node, &tag, 0, nullptr, &tr) == TLAB_OK);      // nvar = 0 reads no field list
        EXPECT(chk(false, 0, 0, 0.5, 1, 1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 0, 0.5, 1, 1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);            // no table
        EXPECT(chk(true, 3, 4, nan, 1, 1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 0, 1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 2, 1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 0, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, -1, -1, 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, -1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, PARTICLE_NP_MAX + 1, l3.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), &node, &tag, -1, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 0, nullptr, nullptr, nullptr, 2, nullptr, nullptr) == TLAB_OK);          // np = 0 reads no pointer
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, nullptr, &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), nullptr, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), &node, nullptr, 2, fl.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), &node, &tag, 2, nullptr, &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), &node, &tag, 2, fhole.data(), &tr) == TLAB_EINVAL);
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, l3.data(), &node, &tag, 2, fl.data(), nullptr) == TLAB_EINVAL);
        EXPECT(chk(true, 6, 4, 0.5, 1, 1, 1, hole.data(), &node, &tag, 2, fl.data(), &tr) == TLAB_EINVAL);         // inertia reads six columns
        EXPECT(chk(true, 3, 4, 0.5, 1, 1, 1, hole.data(), &node, &tag, 1, fhole.data(), &tr) == TLAB_OK);
    }
    if (failures) { std::printf("particles_host_check: %d FAILED\n", failures); return 1; }
    std::printf("particles_host_check ok\n");
    return 0;
}

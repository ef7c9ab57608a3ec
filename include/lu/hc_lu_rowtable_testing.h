/* hc_lu_rowtable_testing.h -- test hook of the fused LU levels' row records
   (csrc/hc_lu_struct.hpp LU_ROWTAB), beside include/lu/hc_lu_testing.h.  The
   throughput tracker's solve reads one record per level and row from LDS where
   it used to rebuild the same values with selects on static lane masks
   (csrc/hc_lu_levels.hpp).  No reference counterpart. */
#ifndef HC_LU_ROWTABLE_TESTING_H
#define HC_LU_ROWTABLE_TESTING_H

#ifdef __cplusplus
extern "C" {
#endif

/* What row `row` (0..31; 30 and 31 are the pad lanes of a half) is to fused
   level `level` (0..3). */
typedef enum {
    HC_LU_ROW_MEMBER = 0,    /* the pivot step of the level whose candidates hold the row; -1: none */
    HC_LU_ROW_BOUND = 1,     /* the fill-in bound of that step, the pattern the row takes (bit c: column c); 0: none */
    HC_LU_ROW_WINDOW = 2,    /* the entry of the half's scratch where its chain's pivot-row window starts;
                                without a member, the row's own window (2 * row) */
    HC_LU_ROW_PARTNER = 3,   /* the row whose triple maximum it takes across a 6-row chain; itself: none */
    HC_LU_ROW_PLACE = 4,     /* its place in its lane triple: row % 3 */
    HC_LU_ROW_CHAIN = 5,     /* the number of its chain among the level's members in increasing step; -1: none */
    HC_LU_ROW_FIELD_COUNT = 6
} hcLuRowField;

/* The field as the kernels decode it from the packed record; -2 for a level,
   row or field out of range. */
int hc_lu_row_field(int level, int row, int field);

#ifdef __cplusplus
}
#endif
#endif /* HC_LU_ROWTABLE_TESTING_H */

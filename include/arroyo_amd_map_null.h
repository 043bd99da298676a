/* The map operator's NULL opcodes: the values of AmdMapInstr.op that follow
 * AMD_MOP_FDIV (20) and are legal only in a program created with
 * AmdMapConfig.null_semantics = 1.  Semantics: the table above enum AmdMapOp
 * in arroyo_amd_types.h, which includes this header; nobody includes it
 * directly.  They are kept apart from enum AmdMapOp: that enum is the opcode
 * set every implementation of the map accepts, the CPU oracle included, and
 * tests/test_cabi.py pins its size; these five exist in the HIP operator
 * alone, and with null_semantics = 0 every value here stays "unknown
 * opcode".  tests/test_mapop_null.py holds them against their twins in
 * arroyo_amd/cabi.py. */
#ifndef ARROYO_AMD_MAP_NULL_H
#define ARROYO_AMD_MAP_NULL_H

enum AmdMapNullOp {
    AMD_MOP_IS_NULL = 21,      /* dst = a is NULL; never NULL */
    AMD_MOP_IS_NOT_NULL = 22,  /* dst = a is valid; never NULL */
    AMD_MOP_COALESCE = 23,     /* dst = a if valid, else b */
    AMD_MOP_NULLIF = 24,       /* dst = NULL if raw a == b, else a */
    AMD_MOP_SELECT = 25        /* dst = a ? b : r[imm]; third source
                                  register in imm */
};

#endif /* ARROYO_AMD_MAP_NULL_H */
